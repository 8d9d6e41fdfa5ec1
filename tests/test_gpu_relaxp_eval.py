"""The points relax engine on the device through its test seams (ochip_relaxp_evaluate, ochip_relaxp_step: obs_kernel,
point_kernel, group_u_kernel, the row owners, mono_kernel, point_prepare_kernel, group_schur_kernel, p_candidate_kernel,
p_slope_kernel, p_reduce_kernel, run by points_model and lm_linear_step) against the long-double oracle of the FULL system
(oracle/relaxp_eval.cpp: nothing eliminated, one dense solve) on the fixtures of tests/relaxp_eval_fixtures.py.

Evaluation: cost, U, g_c, V, g_p and the point-gradient maximum within the normwise bounds, the same unknowns on both sides,
exact zeros where no observation touches.  Step, at radius 1e4 and 1e-2, with the solver's scale and with 1: W and its
right-hand side against the reference's Schur complement; the backward error of the device's own full step in the long-
double system; and, with y_in = the reference's camera step, pt_d, the candidate state, the model cost change, |dx|^2,
|x|^2 and the points' slope.  alpha2 = 0.5 on two cases; the evaluation again after two accepted iterations of the solver.
The bounds and their calibration (never against the device): tests/relaxp_eval_fixtures.py, tests/test_relaxp_eval_oracle.py.
The worst error-to-bound ratios are printed (RELAXP_EVAL_RATIOS).

The device (MI355X) stays at (worst ratio to the bound over all cases): cost 0.0001, U 0.0001, V 0.0001, g_c 0.14, g_p 0.18
and the point-gradient maximum 0.18 (all three: `behind`, whose clamped ray x / 1e-3 amplifies the rounding of x; the fp64
oracle shows the same 0.18), W 0.29, its right-hand side 0.14, pt_d 0.25, the candidate state 0.13, the model cost change
0.14, |dx|^2 0.33 (the candidate is rounded to double before x - candidate is taken, in the fp64 oracle alike), |x|^2
0.00002, the points' slope 0.00001, the backward error of the device's own full step 0.47 (behind, radius 1e-2)."""
import json

import numpy as np
import pytest

import relax_eval_fixtures as G
import relaxp_eval_fixtures as F
from opencalibration_amd import capi

pytestmark = pytest.mark.gpu

RATIOS = {}  # quantity -> (worst ratio, case)
STEPS = [(1e4, None), (1e4, 1.0), (1e-2, None), (1e-2, 1.0)]  # (radius, scale of the reduced unknowns; None: the solver's)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nRELAXP_EVAL_RATIOS " + json.dumps({k: [float(f"{v[0]:.4g}"), v[1]] for k, v in sorted(RATIOS.items())}))


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


_REF = {}


def _ref_eval(oracle, name, scene, structure_only):
    """the long-double evaluation of a case and its bounds, computed once"""
    if name not in _REF:
        ref = oracle.relaxp_eval(scene, precision=1, structure_only=structure_only)
        assert not ref["fail"]
        _REF[name] = (ref, F.eval_bounds(ref))
    return _REF[name]


def _record(r, name):
    print(name, json.dumps({k: float(f"{v:.3g}") for k, v in r.items()}))
    for k, v in r.items():
        if k not in RATIOS or v > RATIOS[k][0]:
            RATIOS[k] = (v, name)


def _to_canonical(ref, dev_order, n_dev):
    """device column of every canonical reduced column; the groups both sides treat as unknowns must be the same"""
    n_cams = len(dev_order) - 8
    perm = np.full(ref["n"], -1)
    for g, size in enumerate([3] * n_cams + [1] * 8):
        co, do = int(ref["order"][g]), int(dev_order[g])
        assert (co >= 0) == (do >= 0), (g, co, do)
        if co >= 0:
            perm[co:co + size] = do + np.arange(size)
    assert n_dev == ref["n"] and np.all(perm >= 0) and len(set(perm)) == len(perm)
    return perm


def _check_eval(ev, ref, b, name):
    perm = _to_canonical(ref, ev["order"], ev["n"])
    got = dict(cost=ev["cost"], U=ev["U"][np.ix_(perm, perm)], g_c=ev["g_c"][perm], V=ev["V"], g_p=ev["g_p"], gmax_p=ev["gmax_p"])
    assert np.array_equal(got["U"], got["U"].T), name
    assert all(np.all(np.isfinite(v)) for v in got.values()), name
    r = F.eval_ratios(got, ref, b)  # (an entry no block touches has bound 0: any error there is an infinite ratio)
    _record(r, name)
    assert all(v <= 1.0 for v in r.values()), (name, r)  # (a NaN ratio fails)
    return perm


@pytest.mark.parametrize("name,scene,structure_only", F.cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_evaluation_against_long_double(ctx, oracle, name, scene, structure_only):
    ref, b = _ref_eval(oracle, name, scene, structure_only)
    _check_eval(ctx.relaxp_evaluate(scene, structure_only=structure_only), ref, b, name)


def _run_step(ctx, oracle, name, scene, structure_only, radius, sc, alpha2=0.0):
    """the device's own step, the reference step (with the backward error of the device's), the device's step again on the
    reference's camera step.  Returns (ref, bounds, perm, L, own, fed, evaluation)"""
    ref, b = _ref_eval(oracle, name, scene, structure_only)
    n = ref["n"]
    scale_c = None if sc is None else np.full(n, sc)
    box = {}

    def second(ev, outs):
        own = outs[0]
        box["perm"] = perm = _to_canonical(ref, ev["order"], ev["n"])
        y_full = np.concatenate([own["y"][perm], (-own["pt_d"] / own["pt_scale"]).reshape(-1)])
        box["L"] = L = oracle.relaxp_step(scene, radius, precision=1, scale_c=scale_c, y_test=y_full, structure_only=structure_only)
        assert not L["fail"]
        y_in = np.zeros(n)
        y_in[perm] = L["y"][:n]
        return dict(radius=radius, scale=scale_c, y_in=y_in, alpha2=alpha2)

    ev, (own, fed) = ctx.relaxp_step(scene, [dict(radius=radius, scale=scale_c), second], structure_only=structure_only)
    return ref, b, box["perm"], box["L"], own, fed, ev


def _assert_solved(own, fed, tag):
    """the factorisation did not fail and nothing the seam returned is NaN or infinite"""
    assert own["fail"] == 0 and fed["fail"] == 0, tag
    for out in (own, fed):
        assert all(np.all(np.isfinite(v)) for v in out.values()), tag


def _check_step(ctx, oracle, name, scene, structure_only, radius, sc):
    ref, b, perm, L, own, fed, ev = _run_step(ctx, oracle, name, scene, structure_only, radius, sc)
    tag = f"{name}@{radius:g}/{'own' if sc is None else sc}"
    n, P = ref["n"], len(scene["point_xyz"])
    sb = F.step_bounds(ref, L, b)
    W = None
    if n:  # (the lower triangle of the device's order holds (i, j) or (j, i) of the canonical one)
        Wd = own["W"][:n]
        full = Wd + np.tril(Wd, -1).T
        W = np.vstack([full[np.ix_(perm, perm)], own["W"][n][perm][None]])
        assert np.array_equal(own["W"], fed["W"]), tag  # the second step of a problem keeps the points' scaling
    got = dict(W=W, pt_d=fed["pt_d"], model_cost_change=fed["model_cost_change"], step_sq=fed["step_sq"], cand_sq=fed["cand_sq"],
               slope_p=fed["slope_p"])
    r = F.step_ratios(got, ref, L, sb)
    # (W as built is judged before the factorisation's flag: a wrong Schur term shows as such, not only as a failed solve)
    assert all(r[k] <= 1.0 for k in ("W", "rhs") if k in r), (tag, {k: r[k] for k in ("W", "rhs") if k in r})
    _assert_solved(own, fed, tag)
    r["backward_error"] = L["backward_error"] / sb["backward_error"]
    # the candidate state
    dxb = np.abs(L["delta"][:n]) * 0.5 * np.diag(b["JtJ"])[:n] / np.maximum(np.diag(ref["JtJ"])[:n], 1e-300) if sc is None else np.zeros(n)
    order = ref["order"]
    n_cams = len(order) - 8
    worst = 0.0
    for c in range(n_cams):
        t = int(order[c])
        bound = F.state_bound(L["cam_q2"][c], np.sum(dxb[t:t + 3]) if t >= 0 else 0.0)
        if t < 0:
            assert np.array_equal(fed["cam_q2"][c], scene["cam_q"][c]), (tag, c)
        worst = max(worst, G.ratio(fed["cam_q2"][c] - L["cam_q2"][c], bound))
    for k in range(8):
        t = int(order[n_cams + k])
        if t < 0:
            assert fed["model2"][k] == scene["model"][k], (tag, k)
        else:
            worst = max(worst, G.ratio(fed["model2"][k] - L["model2"][k], F.state_bound(L["model2"][k], dxb[t])))
    if P:
        worst = max(worst, G.ratio(fed["X2"] - L["X2"], F.state_bound(L["X2"], sb["pt_d"][:, None])))
    r["candidate"] = worst
    _record(r, tag)
    assert all(v <= 1.0 for v in r.values()), (tag, r)  # (a NaN ratio fails)
    return L, fed


@pytest.mark.parametrize("radius,sc", STEPS, ids=lambda v: "own" if v is None else f"{v:g}")
@pytest.mark.parametrize("name,scene,structure_only", F.cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_step_against_long_double(ctx, oracle, name, scene, structure_only, radius, sc):
    L, fed = _check_step(ctx, oracle, name, scene, structure_only, radius, sc)
    if name == "focal_bound" and radius == 1e-2 and sc is None:
        assert L["model2"][0] == scene["focal_hi"] == fed["model2"][0]


def _quat_plus(q, d):
    """EigenQuaternionManifold::Plus (x y z w): (sin|d| / |d| d, cos|d|) * q"""
    nrm = np.linalg.norm(d)
    if nrm == 0.0:
        return np.array(q, float)
    dx, dy, dz = np.sin(nrm) / nrm * d
    dw = np.cos(nrm)
    qx, qy, qz, qw = q
    return np.array([dw * qx + dx * qw + dy * qz - dz * qy, dw * qy + dy * qw + dz * qx - dx * qz,
                     dw * qz + dz * qw + dx * qy - dy * qx, dw * qw - dx * qx - dy * qy - dz * qz])


@pytest.mark.parametrize("name", ["functor3", "roles"])
def test_contracted_step(ctx, oracle, name):
    """alpha2 = 0.5, what the projected line search does: the candidate formed again with fresh = 0 - cameras and lens from
    0.5 times the step, the points from the stored full step - then p_slope_kernel.  The reduced unknowns' scale is 1, so
    the step of a reduced unknown is -0.5 y_in exactly"""
    scene, so = F.case(name)
    ref, b, perm, L, own, fed, ev = _run_step(ctx, oracle, name, scene, so, 1e4, 1.0, alpha2=0.5)
    _assert_solved(own, fed, name)
    n, order = ref["n"], ref["order"]
    n_cams = len(order) - 8
    assert np.array_equal(fed["X2"], scene["point_xyz"] + 0.5 * fed["pt_d"])
    half = -0.5 * L["y"][:n]  # (canonical order; y_in was this y rounded to double)
    parts = [(scene["point_xyz"] - fed["X2"]).reshape(-1)]  # x - candidate over the variable blocks
    cand = [fed["X2"].reshape(-1)]
    for c in range(n_cams):
        t = int(order[c])
        if t < 0:
            assert np.array_equal(fed["cam_q2"][c], scene["cam_q"][c]), (name, c)
            continue
        want = _quat_plus(scene["cam_q"][c], half[t:t + 3])
        assert np.all(np.abs(fed["cam_q2"][c] - want) <= F.state_bound(want)), (name, c)
        parts.append(scene["cam_q"][c] - fed["cam_q2"][c])
        cand.append(fed["cam_q2"][c])
    for first, size in ((0, 1), (1, 2), (3, 3), (6, 2)):
        ts = [int(order[n_cams + first + k]) for k in range(size)]
        for k, t in enumerate(ts):
            want = scene["model"][first + k] + (half[t] if t >= 0 else 0.0)
            assert fed["model2"][first + k] == want, (name, first + k)  # (one product by 0.5, one sum: the same roundings)
        if max(ts) >= 0:  # a variable block counts whole, its constant coordinates included
            parts.append(scene["model"][first:first + size] - fed["model2"][first:first + size])
            cand.append(fed["model2"][first:first + size])
    # |dx|^2 and |x|^2 of the second launch are those of the candidate it wrote: sums of m non-negative terms in another order
    for got, terms in ((fed["step_sq"], np.concatenate(parts) ** 2), (fed["cand_sq"], np.concatenate(cand) ** 2)):
        assert abs(got - terms.sum()) <= 2 * (len(terms) + 2) * G.U * terms.sum(), (name, got, terms.sum())
    sb = F.step_bounds(ref, L, b)
    r = F.step_ratios(dict(pt_d=fed["pt_d"], slope_p=fed["slope_p"]), ref, L, sb)  # (slope_p: p_slope_kernel's g_p . pt_d)
    _record(r, name + "@alpha2")
    assert all(v <= 1.0 for v in r.values()), (name, r)


@pytest.mark.parametrize("name", ["functor3", "roles"])
def test_evaluation_after_accepted_steps(ctx, oracle, name):
    """two iterations of ochip_relaxp_solve, then the evaluation check at the state they leave: the kernels away from the
    seeded state, after steps with the points' scaling fixed"""
    scene, so = F.case(name)
    ev = ctx.relaxp_evaluate(scene, structure_only=so, iterations=2)
    assert ev["summary"]["successful_steps"] >= 1, ev["summary"]
    moved = F.at_state(scene, ev["cam_q"], ev["point_xyz"], ev["model"])
    assert np.abs(moved["point_xyz"] - scene["point_xyz"]).max() > 1e-6
    raw = oracle.relaxp_eval(moved, raw=True, structure_only=so, jacobian=False)
    sq = np.bincount(raw["row_blk"], weights=raw["r"] ** 2)[:2 * len(moved["point_xyz"])]
    assert np.all(np.abs(sq / moved["huber_a"] ** 2 - 1) >= 1e-6)  # (the threshold is still clear at this state)
    ref, b = _ref_eval(oracle, name + "@moved", moved, so)
    _check_eval(ev, ref, b, name + "@moved")


def test_failing_observation_is_reported(ctx, oracle):
    s = F.failing()
    assert oracle.relaxp_eval(s, jacobian=False)["fail"]
    with pytest.raises(capi.OchipError):
        ctx.relaxp_evaluate(s)
