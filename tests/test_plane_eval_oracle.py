"""The plane engine's problems (tests/plane_eval_fixtures.py) through the long-double oracle, on the CPU, before any device
run: the fp64 evaluation inside half of every bound (cost compared as the reduced program's), the bounds failing on
perturbed references, the reduced cost leaving out exactly the blocks that read no unknown, and every Huber decision
clear of its threshold.

The elementwise bound on a block's Jacobian (c u ||J_b||_max, c = 2^18) has a heavy tail over blocks: on the 960 blocks of
the dissected grid, seeds 12, 13, 16 and 18 put one fp64 partial at 1.02, 0.85, 5.3 and 1.5 of it (an angle residual of a
few 1e-6 rad whose camera partials lose ~18 bits in fp64), while J'J and J'r stay at or below 0.0015 of theirs.  Seed 17
(0.27) is used; the device is held to the J'J, J'r and cost bounds only."""
import os

import numpy as np
import pytest

import plane_eval_fixtures as F
import relax_eval_fixtures as G

EDGES = {"huber_above", "huber_below"}  # the deliberate threshold cases: 1e-5 from it


def _all():
    return F.cases() + F.big_cases()


@pytest.fixture(scope="module")
def problems():
    return dict(_all())


@pytest.mark.parametrize("name", [n for n, _ in _all()])
def test_fp64_within_half_of_every_bound(oracle, problems, name):
    s = F.to_relaxg(problems[name])
    ref = oracle.relaxg_eval(s, precision=1)
    d = oracle.relaxg_eval(s, precision=0)
    assert not ref["fail"] and not d["fail"]
    assert np.array_equal(ref["order"], d["order"])
    b = G.bounds(F.reduced(ref))
    r = G.ratios(F.reduced(d), F.reduced(ref), b)
    r["J"] = G.ratio(d["J"] - ref["J"], b["J"])
    assert max(r.values()) <= 0.5, (name, r)


@pytest.mark.parametrize("mutation", ["partial", "drop_block"])
@pytest.mark.parametrize("name", ["plane", "renumbered"])
def test_bounds_fail_on_perturbed_reference(oracle, problems, name, mutation):
    """a partial off by 1e-9 relative and one block missing from the assembly each break a bound (plane: block 0, the
    only block of its pair; a partial of one block of the 200-block pair is below the pair's normwise bound)"""
    s = F.to_relaxg(problems[name])
    ref = oracle.relaxg_eval(s, precision=1)
    b = G.bounds(F.reduced(ref))
    blk = 0 if name == "plane" else 2
    mut, arg = dict(partial=(oracle.MUT_PARTIAL, blk), drop_block=(oracle.MUT_DROP, blk + 1))[mutation]
    m = oracle.relaxg_eval(s, precision=1, mutate=mut, mutate_arg=arg)
    r = G.ratios(F.reduced(m), F.reduced(ref), b)
    assert max(r["JtJ"], r["Jtr"]) > 1.0, (name, mutation, r)


def test_reduced_cost_leaves_out_blocks_without_unknowns(oracle, problems):
    """fixed_pair: the blocks of the constant pair (4, 5) on constant heights and the priors of the constant cameras are
    the whole difference between the cost and the reduced cost; elsewhere only the constant cameras' priors differ"""
    p = problems["fixed_pair"]
    s = F.to_relaxg(p)
    ref = oracle.relaxg_eval(s, precision=1)
    raw = oracle.relaxg_eval(s, precision=1, raw=True)
    nb = len(p["blk_cam_a"])
    sq = np.bincount(raw["row_blk"], weights=raw["r"] ** 2)
    a2 = p["huber_a"] ** 2
    huber = np.where(sq[:nb] > a2, 2 * p["huber_a"] * np.sqrt(sq[:nb]) - a2, sq[:nb]) / 2
    fixed = (p["blk_cam_a"] >= 4) & (p["blk_cam_b"] >= 4)
    assert fixed.sum() == 9
    const_prior = 0.5 * np.sum(sq[nb:][np.asarray(p["cam_optimize"])[p["prior_cam"]] == 0])
    gap = ref["cost"] - ref["cost_reduced"]
    assert gap > 1e6 * G.bounds(F.reduced(ref))["cost"]
    np.testing.assert_allclose(gap, huber[fixed].sum() + const_prior, rtol=1e-12)
    for name in ("plane", "renumbered"):
        e = oracle.relaxg_eval(F.to_relaxg(problems[name]), precision=1)
        assert e["cost_reduced"] <= e["cost"]


def test_cases_reach_their_shapes(oracle, problems):
    """what each case was built for, as the oracle's layout sees it"""
    def n(name, **kw):
        return oracle.relaxg_eval(F.to_relaxg(problems[name]), **kw)["n"]

    assert n("n64") == 64 and n("renumbered") == 192 and n("dissected") == 771 and n("plane") % 64 != 0
    assert n("priors_only") == 3 * 4  # no blocks: no height unknowns
    assert n("plane", structure_only=True) == 2  # (the middle corner is constant)
    p = problems["plane"]
    keys = np.minimum(p["blk_cam_a"], p["blk_cam_b"]) * 100 + np.maximum(p["blk_cam_a"], p["blk_cam_b"])
    assert sorted(np.unique(keys, return_counts=True)[1]) == [1, 63, 64, 65, 200]
    assert np.any(p["blk_cam_a"] > p["blk_cam_b"])


@pytest.mark.parametrize("name", [n for n, _ in _all()])
def test_huber_threshold_is_kept_clear(problems, name):
    """every block's s is at least 1e-6 relative from a^2 (the deliberate edge cases: 1e-5)"""
    m = F.huber_margin(problems[name])
    assert m >= (0.5e-5 if name in EDGES else 1e-6), (name, m)


def test_failing_case_fails(oracle):
    assert oracle.relaxg_eval(F.to_relaxg(F.failing()))["fail"]


@pytest.mark.parametrize("tilt,breaks", [(3e-2, False), (1e-3, True), (1e-4, True), (1e-6, False)])
def test_downward_prior_near_straight_down(oracle, tilt, breaks):
    """camera 6 of plane() is held by its prior alone: at a tilt of 1e-3 - 1e-4 rad from straight down the fp64 evaluation
    itself (the acos of a dot product near 1) is outside the J'J bound; below ~1e-5 the clamp of the dot product at
    1 - 1e-12 zeroes the derivative.  A solve drives such a camera there, so the iterated device cases have none
    (plane_eval_fixtures.plane_iterated)."""
    from relax_fixtures import DOWN, axis_angle, qmul

    p = F.plane()
    q = p["cam_q"].copy()
    q[6] = qmul(DOWN, axis_angle(np.array([0.6, 0.8, 0.0]), tilt))
    s = F.to_relaxg(p, cam_q=q)
    ref, d = oracle.relaxg_eval(s, precision=1), oracle.relaxg_eval(s, precision=0)
    r = G.ratios(F.reduced(d), F.reduced(ref))
    assert (r["JtJ"] > 1.0) == breaks, (tilt, r)


def test_jtr_bound_after_three_steps_is_broken_by_fp64_itself(oracle):
    """the state the device's solve leaves after 3 accepted steps of plane_iterated (tests/golden, recorded from the
    device): block 0, the only block of pair (0, 1), is fitted to ||r_b|| ~ 2e-6, and camera 0's J'r bound (relative to
    ||r_b||) falls below the rounding of its angle residuals.  The fp64 evaluation itself is at 1.7 of that bound there -
    as the device is - while J'J and cost stay far inside theirs; the device cases stop at 2 steps for this case."""
    st = np.load(os.path.join(os.path.dirname(__file__), "golden", "plane_iterated_it3_state.npz"))
    p = F.plane_iterated()
    s = F.to_relaxg(p, st["cam_q"], st["plane_z"])
    ref, d = oracle.relaxg_eval(s, precision=1), oracle.relaxg_eval(s, precision=0)
    r = G.ratios(F.reduced(d), F.reduced(ref))
    assert r["Jtr"] > 1.0 and r["JtJ"] < 1e-3 and r["cost"] < 1e-3, r
    rn0 = np.linalg.norm(ref["r"][ref["row_blk"] == 0])
    assert rn0 < 1e-5, rn0
    at_start = G.ratios(F.reduced(oracle.relaxg_eval(F.to_relaxg(p), precision=0)),
                        F.reduced(oracle.relaxg_eval(F.to_relaxg(p), precision=1)))
    assert at_start["Jtr"] < 0.5, at_start
