"""The long-double evaluation of the general relax engine's problem (oracle/relax_eval.cpp), on the CPU, before any device
run: its Jacobians against its own Richardson-extrapolated central differences, the fp64 evaluation inside half of every
bound of tests/relax_eval_fixtures.py, and the bounds failing on perturbed references.

Calibration of C_BOUND (one constant for cost, J'J, J'r and the block Jacobians; u = 2^-53): at c = 64 the fp64 oracle's
worst ratios over the fixtures were J 976 (mixed_structure_only: the height partials, small against the camera partials the
same functor computes), J'J 354, J'r 41, cost 1.0; c = 2^18 puts every fp64 ratio at or below 0.24.  The device (MI355X,
tests/test_gpu_relax_eval.py) stays at J'J 0.087, J'r 0.010, cost 0.0002 of it."""
import numpy as np
import pytest

import relax_eval_fixtures as F

SMALL = ["mixed", "mixed_fixed_intr", "priors_only", "plane", "tail_f1_pp1_k3", "tail_f0_pp1_k1"]
FD_TOL = 1e-8  # |J - J_fd| <= FD_TOL ||J_b||_max per block (raw residuals)
# The robust centroid of the multi-ray blocks is piecewise (its reweighting and its early exit switch within ~1e-4 of these
# states), so the step is small: at h = 1e-6 the worst difference is 2e-9 of the block's largest partial (long double keeps
# the quotients' rounding near 1e-13); at 1e-4 the multi-ray and intrinsics blocks cross branches.
FD_STEP = 1e-6


def _cases():
    return {name: (s, so) for name, s, so in F.cases()}


@pytest.mark.parametrize("name", SMALL)
def test_jacobian_matches_central_differences(oracle, name):
    s, so = _cases()[name]
    e = oracle.relaxg_eval(s, precision=1, raw=True, structure_only=so)
    assert not e["fail"] and e["n"] > 0
    fd = oracle.relaxg_fd(s, FD_STEP, structure_only=so)
    _, jmax, _, _ = F.block_stats(e)
    tol = FD_TOL * np.maximum(jmax[e["row_blk"]], 1e-300)[:, None]
    err = np.abs(e["J"] - fd)
    worst = np.unravel_index(np.argmax(err / tol), err.shape)
    assert np.all(err <= tol), (name, worst, e["row_blk"][worst[0]], e["J"][worst], fd[worst])


def test_every_functor_family_is_differenced():
    """the fixtures of the difference test hold every block type: 2..5 rays with and without intrinsics and every prior"""
    c = _cases()
    kinds = set()
    for name in SMALL:
        s, _ = c[name]
        for n, i in zip(s["blk_n"], s["blk_intr"]):
            kinds.add((int(n), int(i)))
        for k in ("down_cam", "diff_v", "smooth_v", "rel_cam"):
            if s.get(k) is not None and len(s[k]):
                kinds.add(k)
        if s.get("mono_observations"):
            kinds.add("mono")
        if s["anchor_weight"]:
            kinds.add("anchor")
    assert kinds >= {(n, i) for n in (2, 3, 4, 5) for i in (0, 1)} | {"down_cam", "diff_v", "smooth_v", "rel_cam", "mono", "anchor"}


@pytest.mark.parametrize("name,scene,structure_only", F.cases() + F.big_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_fp64_within_half_of_every_bound(oracle, name, scene, structure_only):
    ref = oracle.relaxg_eval(scene, precision=1, structure_only=structure_only)
    d = oracle.relaxg_eval(scene, precision=0, structure_only=structure_only)
    assert not ref["fail"] and not d["fail"]
    assert np.array_equal(ref["order"], d["order"])
    b = F.bounds(ref)
    r = F.ratios(d, ref, b)
    r["J"] = F.ratio(d["J"] - ref["J"], b["J"])
    assert max(r.values()) <= 0.5, (name, r)


def test_huber_threshold_is_kept_clear():
    """every 2-ray block's s is at least 1e-6 relative from a^2 (the deliberate edge cases 1e-5), and the fixtures hold
    blocks on both sides"""
    from oracle import pyoracle

    sides = set()
    for name, s, so in F.cases() + F.big_cases():
        e = pyoracle.relaxg_eval(s, raw=True, structure_only=so)
        nb = len(s["blk_n"])
        sq = np.bincount(e["row_blk"], weights=e["r"] ** 2)[:nb][s["blk_n"] == 2]
        rel = sq / s["huber_a"] ** 2 - 1
        assert np.all(np.abs(rel) >= 1e-6), (name, np.min(np.abs(rel)))
        sides |= set(np.sign(rel).astype(int))
    assert sides == {-1, 1}


@pytest.mark.parametrize("mutation", ["partial", "no_corrector_on_J", "drop_block"])
def test_bounds_fail_on_perturbed_reference(oracle, mutation):
    """a partial off by 1e-9 relative, the corrector left off J (linear-branch Huber blocks), one block missing from the
    assembly: each breaks a bound"""
    s, _ = _cases()["huber_above"]
    ref = oracle.relaxg_eval(s, precision=1)
    b = F.bounds(ref)
    mut, arg = dict(partial=(oracle.MUT_PARTIAL, 2), no_corrector_on_J=(oracle.MUT_NO_CORR_J, -1),
                    drop_block=(oracle.MUT_DROP, 3))[mutation]
    m = oracle.relaxg_eval(s, precision=1, mutate=mut, mutate_arg=arg)
    r = F.ratios(m, ref, b)
    r["J"] = F.ratio(m["J"] - ref["J"], b["J"])
    assert max(r["JtJ"], r["Jtr"]) > 1.0, (mutation, r)
