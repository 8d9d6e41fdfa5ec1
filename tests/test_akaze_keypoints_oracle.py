"""The restated AKAZE detector and descriptor (oracle/akaze.cpp: determinant maxima, sub-pixel fit, dominant orientation, 486-bit
M-LDB) keypoint by keypoint against the fp64 model of akaze_keypoints_fixtures.py, which is an independent definition-level
check, not OpenCV.  The restatement's own planes (Lt, Lx, Ly) and its own keypoints go in; the scale space is held elsewhere
(test_akaze_planes_oracle.py).  No GPU.

REQUIRED: zero mismatches among decided keypoints and decided bits, on every image.  The caps are conditions on the images, not
results: undecided keypoints (detector, orientation and descriptor together) <= 5 % per image, undecided bits <= 2 % of an
image's bits, and at least 20 isolated decided fp64 candidates on at least three levels of one image, all of them keypoints.

Images: those of the planes work with noisy_176x96 REPLACED by the same size and noise at render_blobs seed 2 - with seed 31 one
of its 19 keypoints is undecided by the detector (its maximum is within 2 eps of a neighbour), 5.3 % against the cap of 5 % -,
plus two that are only checked: graded_640x320 (no image of noise or dense blobs has an isolated candidate above level 1: every
blob is a maximum at every level; the graded image's faint blobs are candidates at level 0, 3 or 7 alone) and dense_640x320
(1801 keypoints, for the device test's partial workgroup).

Observed with the restatement (-s prints them): undecided keypoints 2.4 % / 2.0 % / 1.7 % / 0 % / 0 % / 2.2 %, undecided bits 0.14 % /
0.03 % / 0.02 % / 0 % / 0.16 % / 0.03 % - the share of a descriptor that float32 rounding alone decides -, isolated candidates 15 / 72 / 71
/ 7 / 64 (30 + 22 + 12 on levels 0, 3, 7) / 21, largest angle error among decided keypoints 5.8e-7 rad (ANGLE_TOL 2.3e-6)."""
import numpy as np
import pytest

import akaze_keypoints_fixtures as K
import akaze_planes_fixtures as P

MAX_KP = 40000


@pytest.fixture(scope="module")
def produced(oracle):
    """name -> (the restatement's planes, its keypoints, its descriptors), computed once and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            levels = oracle.akaze_planes(K.image(name))["levels"]
            kp6, desc = oracle.akaze(K.image(name), max_kp=MAX_KP)
            for a in (kp6, desc):
                a.setflags(write=False)
            cache[name] = (levels, kp6, desc)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def checked(produced):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = K.check_image(name, *K.size_of(name), *produced(name))
        return cache[name]

    return get


def test_the_tolerance_is_four_times_what_was_measured():
    assert K.MEASURED_ANGLE_ERROR > 0 and abs(K.ANGLE_TOL / K.MEASURED_ANGLE_ERROR - 4.0) < 1e-9


def test_the_tables():
    """162 comparisons over all 29 cells, every pair of a grid's cells once, the first six the 2 x 2 grid's; 109 samples; the
    weights' centre and corner"""
    picks = K.mldb_picks()
    assert len(picks) == len(set(picks)) == 162 and [p[0][0] for p in picks[:6]] == [2] * 6
    assert sorted(g for (g, _, _), _ in picks) == [2] * 6 + [3] * 36 + [4] * 120
    assert all(a[0] == b[0] and a != b for a, b in picks)
    assert set(K.mldb_picks(forced=False)) == set(picks) and K.mldb_picks(forced=False) != picks
    member, count, comps = K.cells_and_comparisons()
    assert member.shape == (29, 441) and sorted(count) == [25] * 16 + [49] * 9 + [100] * 4 and comps.shape == (162, 2)
    w = K.orientation_weights()
    assert len(K._DISC) == 109 and w[0, 0] == 0.02546481 and w[6, 6] == 0.00008024 and np.array_equal(w, w.T)
    assert abs(K.DELTA_A - 8 * 2.0 ** -21) == 0 and 1.3e-5 < K.DELTA_W < 1.4e-5 and 2.5e-4 < K.delta_p(640, 320) < 2.7e-4


@pytest.mark.parametrize("name", K.IMAGES)
def test_restatement_against_fp64(checked, name):
    r = checked(name)
    iso = r["isolated"]
    print("%s: %d keypoints, %d wrong; undecided keypoints %.2f %% (detector %d, orientation %d, descriptor %d), undecided bits %.3f %%; isolated "
          "candidates %d on levels %s, %d missing; largest angle error %.3g (measured for the tolerance: %.3g)" % (
              name, r["n"], r["wrong"].sum(), 100 * r["undecided_keypoints"], r["undecided_detector"].sum(), r["undecided_orientation"].sum(),
              r["undecided_descriptor"].sum(), 100 * r["undecided_bits"], len(iso), sorted(set(iso[:, 0].tolist())), len(r["missing"]), r["angle_error"],
              K.MEASURED_ANGLE_ERROR))
    assert r["n"] > 0
    assert not r["lines"], "the restatement against the fp64 model:\n" + "\n".join(r["lines"])
    assert not r["wrong"].any()
    assert r["undecided_keypoints"] <= 0.05 and r["undecided_bits"] <= 0.02, (r["undecided_keypoints"], r["undecided_bits"])


def test_isolated_candidates_on_three_levels(checked):
    best = max((checked(name) for name in K.IMAGES), key=lambda r: len(set(r["isolated"][:, 0].tolist())))
    iso = best["isolated"]
    assert len(iso) >= 20 and len(set(iso[:, 0].tolist())) >= 3 and not len(best["missing"]), (len(iso), set(iso[:, 0].tolist()))


def test_the_measured_angle_error(checked):
    worst = max(checked(name)["angle_error"] for name in K.MEASURED_ON)
    print("largest |restatement - model| angle over %s: %.3g rad; stored %.3g, ANGLE_TOL %.3g" % (", ".join(K.MEASURED_ON), worst, K.MEASURED_ANGLE_ERROR, K.ANGLE_TOL))
    assert worst <= K.ANGLE_TOL


STAGE = {m: s for s, ms in (("detector", K.DETECTOR_MUTATIONS), ("orientation", K.ORIENTATION_MUTATIONS), ("descriptor", K.DESCRIPTOR_MUTATIONS)) for m in ms}


@pytest.mark.parametrize("mutation", K.MUTATIONS)
def test_the_margins_have_teeth(produced, mutation):
    """ONE deliberate error in the model shows as mismatches among DECIDED items on at least a tenth of an image's keypoints -
    except cell means instead of sums, which order two cells of one grid alike and must show nothing"""
    assert set(STAGE) == set(K.MUTATIONS)
    shares = {}
    for name in ("noisy_640x320", "noisy_501x334", "blobs_640x320"):
        r = K.check_image(name, *K.size_of(name), *produced(name), mutation=mutation, stages=(STAGE[mutation],))
        shares[name] = float(r["wrong"].mean())
        if shares[name] >= 0.1 or mutation == "cell_means":
            break
    print("%s: keypoints with a mismatch on a decided item: %s" % (mutation, ", ".join("%s %.1f %%" % (k, 100 * v) for k, v in shares.items())))
    if mutation == "cell_means":
        assert max(shares.values()) == 0.0 and not r["lines"], r["lines"]
    else:
        assert max(shares.values()) >= 0.1, shares


def test_the_model_against_long_double(produced):
    """The margins are not the model's own noise: over 200 keypoints every decision margin (TAU of a cell sum, DELTA_W B of a window
    norm, DELTA_A of a sample angle, the sub-pixel bound) is at least 1e3 times the difference between the model in fp64 and in
    long double."""
    name = "noisy_640x320"
    levels, kp6, desc = produced(name)
    kp = np.ascontiguousarray(kp6[::len(kp6) // 200][:200])
    assert len(kp) == 200 and len(set(kp[:, 5].tolist())) >= 4
    table, lv = P.level_table(*K.size_of(name)), K.model_levels(levels)
    ld = np.longdouble
    assert np.finfo(ld).eps < 1e-18, "long double is no wider than double here"
    # cell sums
    _, _, _, a = K.descriptor(table, lv, kp)
    _, _, _, b = K.descriptor(table, lv, kp, dtype=ld)
    assert b["sums"].dtype == ld
    worst = float(np.max(np.abs(a["sums"] - b["sums"]) / a["tau"]))
    print("cell sums: largest |fp64 - long double| / TAU %.3g" % worst)
    assert worst <= 1e-3
    # window norms and sample angles
    a0, _, a = K.orientation(table, lv, kp)
    b0, _, b = K.orientation(table, lv, kp, dtype=ld)
    assert b["norm"].dtype == ld
    worst = float(np.max(np.abs(a["norm"] - b["norm"]) / (K.DELTA_W * a["B"])))
    worst_angle = float(np.max(np.abs(a["samples"] - b["samples"]))) / K.DELTA_A
    print("window norms: largest difference / (DELTA_W B) %.3g; sample angles: / DELTA_A %.3g; keypoint angles: / ANGLE_TOL %.3g" % (
        worst, worst_angle, float(np.max(K.angle_difference(a0, b0))) / K.ANGLE_TOL))
    assert worst <= 1e-3 and worst_angle <= 1e-3 and float(np.max(K.angle_difference(a0, b0))) <= 1e-3 * K.ANGLE_TOL
    # sub-pixel offsets at the pixels the detector check locates
    dets = [K.determinant(l["Lx"], l["Ly"], r["sigma_size"]) for l, r in zip(lv, table)]
    status, _, pix = K.check_detector(table, dets, kp)
    assert (status != K.WRONG).all()
    worst = 0.0
    for i in sorted(set(kp[:, 5].astype(int).tolist())):
        at = pix[kp[:, 5] == i]
        wide = K.determinant(lv[i]["Lx"], lv[i]["Ly"], table[i]["sigma_size"], dtype=ld)
        eps = P.TOLERANCE["Ldet"][i]
        dx, dy, bound = K.subpixel(dets[i], at[:, 0], at[:, 1], eps)
        ex, ey, _ = K.subpixel(wide, at[:, 0], at[:, 1], eps)
        assert ex.dtype == ld
        worst = max(worst, float(np.max(np.maximum(np.abs(dx - ex), np.abs(dy - ey)) / bound)),
                    float(np.max(np.abs(dets[i] - wide)) / eps))
    print("sub-pixel offsets and determinants: largest difference / bound %.3g" % worst)
    assert worst <= 1e-3


def test_measure_oracle_errors(oracle, checked, capsys):
    """measure_oracle_errors() regenerates the stored figure"""
    worst = K.measure_oracle_errors(oracle)
    assert "MEASURED_ANGLE_ERROR" in capsys.readouterr().out
    assert worst == max(checked(name)["angle_error"] for name in K.MEASURED_ON)
    assert 0.5 * K.MEASURED_ANGLE_ERROR <= worst <= 2.0 * K.MEASURED_ANGLE_ERROR, worst          # (another libm moves it a little)
