"""The long-double evaluation and step of the points relax engine's problem (oracle/relaxp_eval.cpp), on the CPU, before any
device run: its Jacobians against its own Richardson-extrapolated central differences, the fp64 evaluation and step inside
half of every bound of tests/relaxp_eval_fixtures.py, and the bounds failing on perturbed references.

FD_TOL and FD_STEP are those of tests/test_relax_eval_oracle.py: the projection is smooth at these states (the clamp of
`behind` is 0.5 m from its switch, the monotonicity samples are clear of zero), so h = 1e-6 serves it as well.

Calibration (u = 2^-53, the fp64 oracle against the long-double one over every fixture; steps at radius 1e4 and 1e-2, with
the solver's scale of the reduced unknowns and with 1).
Evaluation, C_BOUND: at c = 64 the worst ratios were J 3.3 (functor2_k0), J'J 0.57 (functor0), J'r 725 (behind: the
clamped ray is x / 1e-3 with x = 2e-4 left of a subtraction of 0.5 m operands, so its rounding is amplified 2 500 times),
cost 0.44; the existing c = 2^18 puts every fp64 ratio at or below 0.18 and is kept.
Step, each constant at c = 64 and the power of two that puts fp64 at or below 0.5:
  C_W (the Schur term and the damping of W; the U part of W inherits the evaluation bound): W 1.11 (functor0, radius 1e-2,
      scale 1), right-hand side 0.14 -> 2^8 (0.28);
  C_D (pt_d against kappa_p |dp|): 7 690 (sizes, radius 1e4, scale 1: the dense factorisation of all 1 202 unknowns carries
      the conditioning of the whole system into every point, the form only that of the point's own block) -> 2^20 (0.47);
  C_M (model cost change): 1.36 (functor3_k0, radius 1e-2) -> 2^8 (0.34);
  C_N (|dx|^2 and |x|^2): |dx|^2 678 (functor2_k0, radius 1e-2: the damping of the lens columns sits at the 1e-6 floor beside
      columns at 1, and the full solve's error shows in the step's norm), |x|^2 51 -> 2^17 (0.33);
  C_B (backward error of the full step): 7.5 (behind, radius 1e-2) -> 2^10 (0.47);
  the points' slope has no constant of its own (the J'r bound and C_D): fp64 stays at 0.0003."""
import numpy as np
import pytest

import relax_eval_fixtures as G
import relaxp_eval_fixtures as F
from test_relax_eval_oracle import FD_STEP, FD_TOL

SMALL = ["functor0", "functor1", "functor2", "functor3", "functor1_f1_pp0", "functor2_k1", "roles", "behind", "far",
         "mono_active_k1", "mono_active_k3", "focal_bound", "roles_structure_only"]
STEPS = [(1e4, None), (1e4, 1.0), (1e-2, None), (1e-2, 1.0)]  # (radius, scale of the reduced unknowns)


@pytest.mark.parametrize("name", SMALL)
def test_jacobian_matches_central_differences(oracle, name):
    s, so = F.case(name)
    e = oracle.relaxp_eval(s, precision=1, raw=True, structure_only=so)
    assert not e["fail"] and e["N"] > 0
    fd = oracle.relaxp_fd(s, FD_STEP, structure_only=so)
    _, jmax, _, _ = G.block_stats(dict(e, n=e["N"]))
    tol = FD_TOL * np.maximum(jmax[e["row_blk"]], 1e-300)[:, None]
    err = np.abs(e["J"] - fd)
    worst = np.unravel_index(np.argmax(err / tol), err.shape)
    assert np.all(err <= tol), (name, worst, e["row_blk"][worst[0]], e["J"][worst], fd[worst])
    assert not np.any(e["J"][e["touch"] == 0])


def test_every_functor_level_and_the_monotonicity_block_are_differenced(oracle):
    levels, mono_rows = set(), 0
    for name in SMALL:
        s, so = F.case(name)
        levels.add(int(s["functor"]))
        if s["mono_observations"] and s["functor"] >= 2 and not so:
            e = oracle.relaxp_eval(s, precision=1, raw=True)
            rows = e["row_blk"] == 2 * len(s["point_xyz"])
            assert rows.sum() == 10
            active = np.any(e["J"][rows] != 0, axis=1)
            assert 0 < active.sum() < 10, name  # negative at some of the ten samples, positive at others
            mono_rows += int(active.sum())
    assert levels == {0, 1, 2, 3} and mono_rows > 0


def test_huber_threshold_is_kept_clear(oracle):
    """every observation's s is at least 1e-6 relative from a^2 (the deliberate edge cases 1e-5), and every fixture holds
    observations on both sides"""
    for name, s, so in F.cases():
        e = oracle.relaxp_eval(s, raw=True, structure_only=so, jacobian=False)
        sq = np.bincount(e["row_blk"], weights=e["r"] ** 2)[:2 * len(s["point_xyz"])]
        rel = sq / s["huber_a"] ** 2 - 1
        assert np.all(np.abs(rel) >= 1e-6), (name, np.min(np.abs(rel)))
        assert set(np.sign(rel).astype(int)) == {-1, 1}, name
        if name.startswith("huber_"):
            assert abs(np.min(np.abs(rel)) - 1e-5) < 1e-9
    assert F.case("huber_above")[0]["huber_a"] < F.case("huber_below")[0]["huber_a"]


def test_edge_fixtures_hold_their_edges(oracle):
    s, _ = F.case("behind")
    p = int(s["grp_first"][1]) - 1
    ray = F.qrot(F.qinv(s["cam_q"][0]), s["point_xyz"][p] - s["cam_pos"][0])
    assert ray[2] < 1e-3
    e = oracle.relaxp_eval(s, precision=1, raw=True)
    n = e["n"]
    Jp = e["J"][e["row_blk"] == 2 * p][:, n + 3 * p:n + 3 * p + 3]
    assert np.allclose(Jp @ F.qrot(s["cam_q"][0], [0, 0, 1.0]), 0, atol=1e-9 * np.abs(Jp).max())  # no depth partial
    s, _ = F.case("far")
    p = int(s["grp_first"][1]) - 1
    st = oracle.relaxp_step(s, 1e4)
    e = oracle.relaxp_eval(s, jacobian=False)
    cols = e["n"] + 3 * p + np.arange(3)
    assert np.all(np.diag(e["JtJ"])[cols] * st["scale"][cols] ** 2 < 1e-6) and np.allclose(st["D2"][cols], 1e-6 / 1e4)
    s, _ = F.case("focal_bound")
    st = oracle.relaxp_step(s, 1e-2)
    assert st["model2"][0] == s["focal_hi"] and s["model"][0] + st["delta"][oracle.relaxp_eval(s, jacobian=False)["order"][5]] > 1000.9
    s, _ = F.case("sizes")
    assert list(np.diff(s["grp_first"])) == [1, 63, 64, 65, 200]
    assert F.case("wide")[0]["cam_pos"].shape[0] * 3 + 8 > 64
    assert oracle.relaxp_eval(F.failing(), jacobian=False)["fail"]


@pytest.mark.parametrize("name,scene,structure_only", F.cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_fp64_within_half_of_every_bound(oracle, name, scene, structure_only):
    ref = oracle.relaxp_eval(scene, precision=1, structure_only=structure_only)
    d = oracle.relaxp_eval(scene, precision=0, structure_only=structure_only)
    assert not ref["fail"] and not d["fail"]
    assert np.array_equal(ref["order"], d["order"])
    b = F.eval_bounds(ref)
    r = G.ratios(d, ref, b)
    r["J"] = G.ratio(d["J"] - ref["J"], b["J"])
    n = ref["n"]
    for radius, sc in STEPS:
        scale_c = None if sc is None else np.full(n, sc)
        L = oracle.relaxp_step(scene, radius, precision=1, scale_c=scale_c, structure_only=structure_only)
        D = oracle.relaxp_step(scene, radius, precision=0, scale_c=scale_c, structure_only=structure_only)
        assert not L["fail"] and not D["fail"]
        sb = F.step_bounds(ref, L, b)
        got = dict(W=np.vstack([D["Sc"], D["rhs_c"][None]]) if n else None, pt_d=D["delta"][n:].reshape(-1, 3),
                   model_cost_change=D["model_cost_change"], step_sq=D["step_sq"], cand_sq=D["cand_sq"], slope_p=D["slope_p"])
        for k, v in F.step_ratios(got, ref, L, sb).items():
            r[k] = max(r.get(k, 0.0), v)
        be = oracle.relaxp_step(scene, radius, precision=1, scale_c=scale_c, y_test=D["y"], structure_only=structure_only)
        r["backward_error"] = max(r.get("backward_error", 0.0), be["backward_error"] / sb["backward_error"])
    assert max(r.values()) <= 0.5, (name, r)


@pytest.mark.parametrize("mutation", ["partial", "no_corrector_on_J", "drop_schur_point", "no_point_damping"])
def test_bounds_fail_on_perturbed_reference(oracle, mutation):
    """a partial off by 1e-9 relative, the corrector left off J (linear-branch observations), one point missing from the Schur
    term, the damping left off the point blocks: each breaks a bound"""
    s, _ = F.case("huber_above")
    ref = oracle.relaxp_eval(s, precision=1)
    b = F.eval_bounds(ref)
    mut, arg = dict(partial=(oracle.PMUT_PARTIAL, 2), no_corrector_on_J=(oracle.PMUT_NO_CORR_J, -1),
                    drop_schur_point=(oracle.PMUT_DROP_SCHUR, 3), no_point_damping=(oracle.PMUT_NO_POINT_DAMPING, -1))[mutation]
    if mutation in ("partial", "no_corrector_on_J"):
        m = oracle.relaxp_eval(s, precision=1, mutate=mut, mutate_arg=arg)
        r = G.ratios(m, ref, b)
        assert max(r["JtJ"], r["Jtr"]) > 1.0, (mutation, r)
        return
    n = ref["n"]
    L = oracle.relaxp_step(s, 1e4, precision=1)
    M = oracle.relaxp_step(s, 1e4, precision=1, mutate=mut, mutate_arg=arg)
    got = dict(W=np.vstack([M["Sc"], M["rhs_c"][None]]), pt_d=M["delta"][n:].reshape(-1, 3))
    r = F.step_ratios(got, ref, L)
    assert (r["W"] if mutation == "drop_schur_point" else min(r["W"], r["pt_d"])) > 1.0, (mutation, r)
