"""The restated AKAZE scale space (oracle/akaze.cpp, all planes of one build through oc_akaze_planes) against the fp64 model of
akaze_planes_fixtures.py, plane by plane and level by level, and against answers that need no model.  No GPU.

What the table in the fixtures module holds (max |oracle - model| over every pixel, worst over the four images; allowed is 4 x):
    Lt    2.4e-7 - 3.4e-7 at levels 0 - 11, 6.1e-7 / 3.1e-7 / 3.4e-7 / 8.5e-7 at levels 12 - 15 (80 x 40: fp32 round-off amplified
          by FED cycles of 17 - 29 steps)
    Lx    2.0e-8 - 5.4e-8        Ly    1.8e-8 - 5.3e-8        Ldet  2.1e-9 - 3.2e-8
    mean(Lt[i]) - mean(Lt[0]), shapes that halve exactly: at most 3.0e-9
Run with -s to see every observed figure next to its entry."""
import numpy as np
import pytest

import akaze_planes_fixtures as F

# the contrast factor's histogram bin per image: fp64 and fp32 pick the same one for these seeds (asserted below)
K_BINS = {"blobs_640x320": 52, "noisy_640x320": 25, "noisy_501x334": 20, "noisy_176x96": 38}


@pytest.fixture(scope="module")
def planes(oracle):
    """name -> (the oracle's planes, the model's with the oracle's contrast factor, the model's own contrast factor), computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            o = oracle.akaze_planes(F.image(name))
            m = F.scale_space(F.image(name), kcontrast=float(o["kcontrast"]))
            cache[name] = (o, m)
        return cache[name]

    return get


def test_the_table_is_four_times_what_was_measured():
    for p in F.PLANES:
        assert len(F.MEASURED_AND_ALLOWED[p]) == 16
        for measured, allowed in F.MEASURED_AND_ALLOWED[p]:
            assert measured > 0 and abs(allowed / measured - 4.0) < 1e-9


@pytest.mark.parametrize("name", list(F.IMAGES))
def test_level_table(planes, name):
    o, m = planes(name)
    w, h = F.IMAGES[name][:2]
    assert len(o["levels"]) == len(m["levels"]) == {640: 16, 501: 12, 176: 8}[w]
    for a, b in zip(o["levels"], m["levels"]):
        for key in ("octave", "sublevel", "width", "height", "sigma_size"):
            assert a[key] == b[key], (key, a[key], b[key])
        assert abs(a["esigma"] / b["sigma"] - 1) < 3e-7 and abs(a["etime"] / b["etime"] - 1) < 5e-7      # float32 of 1.6f * powf(2, .)
    assert (o["levels"][-1]["width"], o["levels"][-1]["height"]) == {640: (80, 40), 501: (125, 83), 176: (88, 48)}[w]
    n = [l["n_steps"] for l in o["levels"]]
    assert n == [0] + [len(F.fed_steps(b["etime"] - a["etime"])) for a, b in zip(m["levels"], m["levels"][1:])]


@pytest.mark.parametrize("name", list(F.IMAGES))
def test_oracle_planes_against_fp64(planes, name):
    o, m = planes(name)
    errors = F.max_errors(o["levels"], m["levels"])
    for p in F.PLANES:
        print("%s %-4s observed / measured-for-the-table:" % (name, p), " ".join("%.2g/%.2g" % (e, F.MEASURED[p][i]) for i, e in enumerate(errors[p])))
    bad = F.tolerance_report(errors)
    assert not bad, "%s: %d planes beyond 4 x the measured error:\n%s" % (name, len(bad), "\n".join(bad))


@pytest.mark.parametrize("mutation", F.MUTATIONS)
def test_the_tolerances_have_teeth(planes, mutation):
    """every deliberate error in the model misses the table by a factor of 100 at some (level, plane): a condition on the table"""
    o, _ = planes("noisy_640x320")
    wrong = F.scale_space(F.image("noisy_640x320"), kcontrast=float(o["kcontrast"]), mutation=mutation)
    errors = F.max_errors(o["levels"], wrong["levels"])
    ratio, level, plane = max((errors[p][i] / F.TOLERANCE[p][i], i, p) for p in F.PLANES for i in range(16))
    first = min((i, p) for p in F.PLANES for i in range(16) if errors[p][i] > F.TOLERANCE[p][i])
    print("%s: %.3g x the tolerance at level %d %s; first beyond it: level %d %s" % ((mutation, ratio, level, plane) + first))
    assert ratio >= 100.0, "%s reaches only %.3g x the tolerance (level %d %s): the table is too wide" % (mutation, ratio, level, plane)


def test_the_model_against_long_double():
    """the model's own round-off is nothing against the table: fp64 and long double agree to 1e-6 of the smallest entry (a model
    that takes a FED cycle's steps in ascending order is 4.9e-5 off at level 15)"""
    a =F.scale_space(F.image("noisy_640x320"), kcontrast=0.48)
    b = F.scale_space(F.image("noisy_640x320"), kcontrast=0.48, dtype=np.longdouble)
    errors = F.max_errors(b["levels"], a["levels"])
    assert b["levels"][-1]["Lt"].dtype == np.longdouble
    for p in F.PLANES:
        print(p, " ".join("%.2g" % e for e in errors[p]))
        assert max(errors[p]) <= 1e-6 * min(F.TOLERANCE[p])


@pytest.mark.parametrize("name", list(F.IMAGES))
def test_contrast_factor(planes, name):
    """The model's own factor against the oracle's: the same histogram bin k, and hmax k / 300 equal to float32 rounding - the ~ 10
    roundings of the Gaussian, the Scharr sums, the magnitude and the two final operations, 6e-8 each: 1e-6; the next bin is 1 / k >=
    2 % away."""
    o, _ = planes(name)
    own = F.scale_space(F.image(name))
    k_oracle = float(o["kcontrast"]) * 300.0 / own["hmax"]
    print("%s: oracle %.9g, model %.9g (bin %d, hmax %.9g), relative %.3g" % (name, o["kcontrast"], own["kcontrast"], own["k_bin"], own["hmax"],
                                                                           abs(o["kcontrast"] / own["kcontrast"] - 1)))
    assert own["k_bin"] == K_BINS[name] == int(round(k_oracle)), (own["k_bin"], k_oracle)
    assert abs(float(o["kcontrast"]) / own["kcontrast"] - 1.0) < 1e-6


def test_constant_image(oracle):
    """no structure: Lt exactly constant, Lx, Ly, Ldet exactly zero at every level, and the blank image's contrast factor"""
    o = oracle.akaze_planes(F.constant_image(640, 320, 127))
    assert len(o["levels"]) == 16 and o["kcontrast"] == np.float32(0.03)
    for i, l in enumerate(o["levels"]):
        assert np.all(l["Lt"] == l["Lt"][0, 0]) and abs(float(l["Lt"][0, 0]) - 127 / 255) < 1e-6, i
        for p in ("Lx", "Ly", "Ldet"):
            assert not l[p].any(), (i, p)
    m = F.scale_space(F.constant_image(640, 320, 127))
    assert m["kcontrast"] == 0.03 and all(np.ptp(l["Lt"]) < 1e-15 and np.abs(l["Ldet"]).max() < 1e-30 for l in m["levels"])


@pytest.mark.parametrize("name", F.EXACT_HALVING)
def test_the_mean_is_preserved(planes, name):
    """no flux through the border and a 2 x 2 mean between the octaves: every level's mean is level 0's"""
    o, m = planes(name)
    drift = [abs(l["Lt"].astype(np.float64).mean() - o["levels"][0]["Lt"].astype(np.float64).mean()) for l in o["levels"]]
    print("%s: mean drift per level" % name, " ".join("%.2g" % d for d in drift), "(measured for the bound: %.2g)" % F.MEASURED_MEAN_DRIFT)
    assert max(drift) <= F.MEAN_DRIFT_TOLERANCE, (max(drift), int(np.argmax(drift)))
    assert max(abs(l["Lt"].mean() - m["levels"][0]["Lt"].mean()) for l in m["levels"]) < 1e-14        # (the model: exactly, to fp64)


def ramp_margins(levels):
    """Per level, the columns from each side within which the replicated / reflected border can be felt: (Lt, derivatives).  Every
    operation has compact support: Gaussian(1.6) 4 columns, Gaussian(1) 2, the conductivity's Scharr 1, a diffusion step 1 (the
    steps leave a linear image alone where the conductivity is constant around it), the 2 x 2 mean halves, the derivative s."""
    out, m = [(4, 4 + levels[0]["sigma_size"])], 4
    for p, l in zip(levels, levels[1:]):
        if l["octave"] > p["octave"]:
            m = (m + 1) // 2
        out.append((m + 4 + l["n_steps"], m + 2 + l["sigma_size"]))
        m = out[-1][0]
    return out


def test_horizontal_ramp(oracle):
    """A linear image is a fixed point of the diffusion: away from the left and right borders Lt stays the ramp (the 2 x 2 mean of
    it in the second octave), Lx is 2^octave times the slope, and everywhere Ly and Ldet are exactly zero (every row is the same).
    Bounds: Lt 2e-6 - the two Gaussian passes' float32 taps and sums, 5e-7 on values up to 1, and half an ulp, 3e-8, for each of
    the 32 diffusion steps up to the last level; Lx 1e-6: the differences of two such values over 2 s >= 4 pixels, which is
    2.6e-4 of the slope."""
    grey = F.ramp_image(256, 96)
    o = oracle.akaze_planes(grey)
    levels = o["levels"]
    assert len(levels) == 8 and sum(l["n_steps"] for l in levels) == 32
    slope = 1.0 / 255.0
    for i, (l, (m_lt, m_d)) in enumerate(zip(levels, ramp_margins(levels))):
        w, step = l["width"], 1 << l["octave"]
        assert w - 2 * max(m_lt, m_d) >= 16, (i, w, m_lt, m_d)           # (columns are left to look at)
        x = np.arange(w, dtype=np.float64)
        want = (x * step + 0.5 * (step - 1)) * slope
        e_lt = np.abs(l["Lt"][:, m_lt:w - m_lt] - want[None, m_lt:w - m_lt]).max()
        e_lx = np.abs(l["Lx"][:, m_d:w - m_d].astype(np.float64) - step * slope).max()
        print("level %d: columns %d / %d from the border on, |Lt - ramp| %.2g, |Lx - %d slope| %.2g" % (i, m_lt, m_d, e_lt, step, e_lx))
        assert e_lt <= 2e-6 and e_lx <= 1e-6, (i, e_lt, e_lx)
        assert not l["Ly"].any() and not l["Ldet"].any(), i
