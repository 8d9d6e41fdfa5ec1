"""homography_model::decompose on the CPU, before any device run: the host route (csrc/decompose.hpp through
och_homography_decompose) and the oracle's restatement (oracle/ransac.cpp) on homographies built from known motions
(tests/decompose_fixtures.py) - the motion comes back inside the error model, the vote counts and the order are the expected
ones, the two routes are equal to the bit - and csrc/decompose.hpp's order_by_votes and quaternion_from_rotation in a
stand-alone program against std::stable_sort and the rotation rebuilt from q (decompose_order_driver.cpp, under the address
and undefined-behaviour sanitizers where they link; nothing loaded into Python runs under a sanitizer).

Calibration of C_DEC (one constant for |R(q) - R|, |t_out -+ t| / max(tau, 1), the rank-one residual and | |q| - 1 |),
E = C_DEC 2^-24 / (min(1, tau^2) gamma) + C_DEC 2^-53 kappa(H), fp64 oracle on the 523 bounded motions of the fixtures,
worst ratio per quantity at C = 1: rank one 2.56 (general374, tau 2.44), t 1.65 (general364, tau 1.81), R 1.60
(rotation_yaw90: 1.6 u on an exact rotation), q 0.27.  The smallest power of two that puts every ratio at or below 0.5 is
C_DEC = 2^3.  The model needed no further factor: the large ratios sit at tau > 1, where v = 2 sqrtf(..) is about
2 (1 + gamma) and its single-precision rounding grows with it; no case with two nearly equal |S_ii| stands out.

Host and oracle are equal to the bit on every fixture (542 motions, 18 degenerate matrices, 78 vote jobs), after the oracle's
Jacobi sweep took the sign of theta = -0.0 as the header does (one ulp of sigma_2 on -R, R a drawn rotation); that stronger
bar is what is asserted.  Branch and sign coverage of the 472 general motions past the pure-rotation shortcut (truth, long
double): |S00| largest 75 with e12 > 0 and 73 with e12 < 0, |S11| largest 74 / 75 by e02, |S22| largest 90 / 85 by e01.

What is agreement-only and why:
  a pure climb (t parallel to n) has S of rank one - every 2 x 2 minor is 0 in truth, so rounding decides each sign and
  whether a minor under its square root is negative: of the six climbs one (climb3) returns NaN poses on every route, the
  others finite ones.  OpenCV does the same; nothing is clamped, the routes agree.
  the pure-rotation shortcut under a negative scale returns -R (no rotation; OpenCV's behaviour, kept).
  yaw at a multiple of 90 degrees with the translation along an image axis (a zero minor under the square root).
DECOMP_RATIOS {"R": {"ratio": 0.2, "job": "rotation_yaw90"}, "t": {"ratio": 0.207, "job": "general364"}, "rank1": {"ratio": 0.32, "job": "general374"}, "q": {"ratio": 0.0333, "job": "general364"}}"""
import json
import os
import subprocess
import warnings

import numpy as np
import pytest

import decompose_fixtures as F
from homography_fit_fixtures import UNIT, corr7, rays_of
from opencalibration_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- order_by_votes and quaternion_from_rotation in a stand-alone program ------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("decompose_order") / "driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-o", exe,
           os.path.join(HERE, "decompose_order_driver.cpp")]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:
        warnings.warn("the sanitizer runtimes do not link here: the driver runs plain")
        subprocess.run(cmd, check=True)
    return exe


def test_order_and_quaternion_branches(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "625 rows equal std::stable_sort" in r.stdout and "clean" in r.stdout
    print(r.stdout)


# ---- both routes on every fixture ----------------------------------------------------------------------------------------
def _both(oracle, H, r1, r2, flags):
    """(can_decompose, poses) of the host and of the oracle"""
    f = np.asarray(flags, bool)
    with np.errstate(all="ignore"):
        h = host.decompose(H, r1[f], r2[f])
        o = oracle.decompose(H, corr7(r1, r2), flags) if len(r1) else oracle.decompose(H, np.zeros((1, 7)), np.zeros(1, np.uint8))
    return h, o


@pytest.fixture(scope="module")
def motion_runs(oracle):
    """every motion and degenerate matrix with the common rays, all flagged: name -> (case, host result, oracle result)"""
    p1, p2 = F.common_pixels()
    r1, r2 = rays_of(p1, UNIT), rays_of(p2, UNIT)
    return {c["name"]: (c,) + _both(oracle, c["H"], r1, r2, np.ones(len(r1), np.uint8)) for c in F.motions() + F.degenerate()}


def test_rays_equal_the_oracles(oracle):
    model = np.concatenate([UNIT, [4000.0, 3000.0]])
    for j in F.votes():
        for px in (j["px1"], j["px2"]):
            if len(px):
                assert np.array_equal(oracle.image_to_3d(px, model), rays_of(px, UNIT), equal_nan=True), j["name"]
    for px in F.common_pixels():
        assert np.array_equal(oracle.image_to_3d(px, model), rays_of(px, UNIT))


def test_host_equals_oracle_bit_for_bit(motion_runs):
    """number of solutions, every NaN position, scores, order, can_decompose - and the poses themselves"""
    bad = [name for name, (c, (okh, ph), (oko, po)) in motion_runs.items() if okh != oko or not F._same_bits(ph, po)]
    assert not bad, bad


def test_bounded_motions_come_back_within_half_the_bound(motion_runs):
    """the calibration of C_DEC: the truth among the four poses, twins, rank one, |q| = 1, all inside E / 2; no NaN"""
    bad, worst, n = [], F.Worst(), 0
    for name, (c, (okh, ph), (oko, po)) in motion_runs.items():
        if not c["bounded"]:
            continue
        n += 1
        for route, p in (("host", ph), ("oracle", po)):
            if np.isnan(p[:c["solutions"], :7]).any():
                bad.append((route, name, "NaN"))
                continue
            problems, r = F.check_poses(c, p)
            worst.add(name, r)
            if problems or max(r.values()) > 0.5 or F.check_order(p):
                bad.append((route, name, problems, r))
    print("DECOMP_RATIOS " + worst.line())
    print("DECOMP_CALIBRATION C_DEC=%g, %d bounded motions, worst fp64 ratios at C = 1: %s; coverage (branch, sign): %s"
          % (F.C_DEC, n, {k: ("%.3g" % (v[0] * F.C_DEC), v[1]) for k, v in worst.w.items()}, F.coverage()))
    assert n >= 500 and not bad, bad[:10]


def test_agreement_only_cases_are_reported(motion_runs):
    """what the routes return where no bound applies (they agree: test_host_equals_oracle_bit_for_bit).  The pure climbs are
    the documented NaN: at least one climb is finite, and a NaN never comes alone - q, t of all four poses or none"""
    seen = {}
    for name, (c, (okh, ph), _) in motion_runs.items():
        if c["bounded"]:
            continue
        nan = np.isnan(ph[:, :7])
        seen[name] = "NaN" if nan.all() else "finite" if not nan.any() else "%d solutions" % int((~nan.any(1)).sum())
        assert not F.check_order(ph) or nan.all(), (name, ph[:, 7])
    print("DECOMP_AGREEMENT_ONLY " + json.dumps(seen))
    climbs = [v for k, v in seen.items() if k.startswith("climb")]
    assert "finite" in climbs and set(climbs) <= {"finite", "NaN"}, climbs
    for k in ("zero", "all_nan", "nan_entry", "inf_entry"):
        assert not motion_runs["degenerate_" + k][1][0], k   # can_decompose


def test_the_bound_bites():
    """a pose 4 E off the truth - the rotation turned, the translation stretched - leaves the bound on every bounded case"""
    tried = 0
    for c in F.general()[::20]:
        E = F.bound(c)
        if not c["bounded"] or c["solutions"] != 4 or E > 1e-3:
            continue
        for what in ("R", "t"):
            R = F.rotation([0, 0, 1], 6 * E) @ c["R"] if what == "R" else c["R"]
            t = c["t"] * (1 + 4 * E * max(c["tau"], 1) / c["tau"]) if what == "t" else c["t"]
            m = np.array(R.astype(np.float64))
            q = np.zeros(4)
            w = np.sqrt(max(0.0, 1 + m[0, 0] + m[1, 1] + m[2, 2])) / 2
            if w < 0.1:   # (the plain formula below is for angles away from pi)
                continue
            tried += 1
            q[:] = [(m[2, 1] - m[1, 2]) / (4 * w), (m[0, 2] - m[2, 0]) / (4 * w), (m[1, 0] - m[0, 1]) / (4 * w), w]
            poses = np.zeros((4, 8))
            for k in range(4):
                poses[k, :4] = q if k < 2 else [q[1], -q[0], q[3], -q[2]]
                poses[k, 4:7] = (t if k % 2 == 0 else -t).astype(np.float64)
            problems, r = F.check_poses(c, poses)
            assert r[what] > 1, (c["name"], what, r)
    assert tried >= 10, tried


# ---- the vote and the order ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vote_solutions(oracle):
    """the solutions of the two vote matrices in the decomposition's order, from runs without a vote"""
    out = {}
    for j in F.votes():
        name = j["case"]["name"]
        if name not in out:
            (okh, ph), (oko, po) = _both(oracle, j["case"]["H"], np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.uint8))
            assert not okh and not oko and F._same_bits(ph, po)
            out[name] = F.solutions_by_index(ph)
    return out


def test_votes_scores_order_and_can_decompose(oracle, vote_solutions):
    bad, patterns = [], set()
    for j in F.votes():
        r1, r2 = F.job_rays(j)
        can, rows, score = F.expected_rows(j["case"]["H"], vote_solutions[j["case"]["name"]], r1, r2, j["flags"])
        for route, (ok, p) in zip(("host", "oracle"), _both(oracle, j["case"]["H"], r1, r2, j["flags"])):
            if ok != can or not F._same_bits(p, rows):
                bad.append((route, j["name"], ok, can, p[:, 7].tolist(), rows[:, 7].tolist()))
        patterns.add(tuple(score))
    assert not bad, bad[:10]
    # the tie patterns the rows realise, in solution order before the sort
    shapes = {tuple(int(np.sign(s)) for s in p) for p in patterns if len({s for s in p if s > 0}) == 1}
    assert {(1, 0, 1, 0), (1, 0, 0, 1), (0, 1, 1, 0), (0, 1, 0, 1), (1, 1, 1, 1)} <= shapes, shapes
    assert (0, 0, 0, 0) in patterns and (0, -1, -1, -1) in patterns
    assert any(p[0] > 0 and p[1:] == (-1, -1, -1) for p in patterns)
    assert any(len(set(p)) == 4 for p in patterns)   # and a row without a tie
    print("DECOMP_VOTE_PATTERNS %d distinct score rows" % len(patterns))


def test_vote_motion_is_held_like_the_others(oracle, vote_solutions):
    c = F.vote_motion()
    poses = np.zeros((4, 8))
    poses[:, :7] = vote_solutions[c["name"]]
    problems, r = F.check_poses(c, poses)
    assert not problems and max(r.values()) <= 0.5, (problems, r)
