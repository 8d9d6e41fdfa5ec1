"""The references of the chain trace tests (tests/test_gpu_chain_trace.py) checked without a device, before any device run:
for every scene of tests/chain_fixtures.py and every step of it (at the state the step starts from when no solve has
moved a camera), the set-up restated in numpy, the first evaluation of both solves by the fp64 oracle and the first linear
solve in fp64 numpy (n <= 12: the transcription of the chain's one-thread Cholesky; above: LAPACK's) are inside HALF of
every bound the device is held to against the long-double reference; every comparison fails when the "device" value is
moved by a few bound-widths (one J'J entry, one transposed 3 x 3 pair block, one chunk's contribution dropped, one factor
entry, the damping added before the scaling instead of after it); every Huber decision and every grid-filter score is
clear of a tie, except in the hand-over scene.

The constants are the project's: relax_eval_fixtures.C_BOUND = 2^18, lm_fixtures' 4, 32 u for the quaternion step.  None
was calibrated here or on the device's numbers; a fixture that cannot keep the fp64 reference within half of a bound is
to be changed, not the constant."""
import numpy as np
import pytest

import chain_fixtures as F
import lm_fixtures as LM
import plane_eval_fixtures as P
import relax_eval_fixtures as G
from opencalibration_amd import host

SCENES = F.scenes()
STEPS = [(name, i) for name, s in SCENES.items() for i in range(len(s.steps))]


def _rays(arr):
    inl = arr["inliers"]
    return np.concatenate([host.image_to_3d(inl["px1"], F.MODEL10), host.image_to_3d(inl["px2"], F.MODEL10)], 1)


def _start(scene, upto):
    """the state step `upto` starts from when no solve has moved a camera: the orientations taken over so far"""
    q = scene.cam_q.copy()
    for st in scene.steps[:upto + 1]:
        if st["mode"] != 2:
            q[st["cam"]] = q[st["prev_cam"]] if st["prev_cam"] >= 0 else st["prev_q"]
    return q


@pytest.fixture(scope="module")
def cases(oracle):
    """(scene, step) -> the numpy set-up and, per solve (0: heights alone, 1: with cameras), the plane problem, the fp64 and
    the long-double evaluation and the column map; computed once"""
    out = {}
    for name, i in STEPS:
        s = SCENES[name]
        arr = s.arrays()
        rays = _rays(arr)
        q = _start(s, i)
        su = F.setup_numpy(arr, rays, q, s.steps[i]["n_filter"])
        sn = F.step_numpy(arr, arr["steps"][i], q, su["blk_idx"])
        solves = {}
        for which in (0, 1):
            cam_t = sn["cam_t"] if which else np.full(len(q), -1)
            n_active = int((cam_t >= 0).sum())
            nz = 3 if sn["n_blocks"] else 0
            if 3 * n_active + nz == 0:
                continue
            p = F.plane_problem(arr, rays, su["blk_idx"], q, np.full(3, F.Z0), cam_t, sn["cam_prior"], which)
            scene = P.to_relaxg(p)
            ref = oracle.relaxg_eval(scene, precision=1, structure_only=not which)
            d = oracle.relaxg_eval(scene, precision=0, structure_only=not which)
            solves[which] = dict(p=p, ref=ref, d=d, cam_t=cam_t, n_active=n_active, nz=nz,
                                 perm=F.columns(ref["order"], cam_t, n_active, nz, ref["n"]))
        out[(name, i)] = dict(arr=arr, rays=rays, q=q, setup=su, step=sn, solves=solves)
    return out


def _chain_order(e, perm):
    """an oracle evaluation's J'J and J'r in the chain's column order"""
    n = len(perm)
    A, g = np.zeros((n, n)), np.zeros(n)
    A[np.ix_(perm, perm)] = e["JtJ"]
    g[perm] = e["Jtr"]
    return A, g


def test_the_scenes_reach_the_paths_they_are_built_for(cases):
    n_of = {}
    for (name, i), c in cases.items():
        n_of[(name, i)] = {w: 3 * v["n_active"] + v["nz"] for w, v in c["solves"].items()}
    assert n_of[("bootstrap", 0)] == {1: 3} and cases[("bootstrap", 0)]["step"]["n_blocks"] == 0  # the prior alone, no heights
    assert n_of[("bootstrap", 1)] == {0: 3, 1: 6} and n_of[("bootstrap", 2)] == {0: 3, 1: 12} and n_of[("bootstrap", 3)][1] == 12
    for name, n in (("n12", 12), ("n15", 15), ("n63", 63), ("n66", 66), ("n129", 129)):
        assert n_of[(name, 0)] == {0: 3, 1: n}, (name, n_of[(name, 0)])
    c = cases[("bootstrap", 1)]
    counts = [len(l) for l in c["setup"]["blk_idx"]]
    assert counts == [1, 63, 64, 65, 130, 7, 0, 9, 6, 0], counts  # the dead edge and the one behind n_filter: no block
    e = c["arr"]["edges"]
    assert (e["cam_a"][0], e["cam_b"][0]) == (1, 0) and (e["cam_a"][1], e["cam_b"][1]) == (0, 1)  # both orders, cam_a > cam_b
    assert c["step"]["n_live"] == 1 + 1 + 1 + 2 + 3 + 1 + 0 + 1 + 1 and np.isnan(c["q"][5]).all()
    s12 = cases[("n12", 0)]["step"]
    assert s12["cam_prior"][4] and not s12["cam_blocks"][4] and s12["cam_t"][4] == 6  # held by its prior alone
    assert len(SCENES["n129"].cam_pos) <= 45


def test_no_score_and_no_huber_decision_is_near_a_tie(cases):
    for key, c in cases.items():
        assert c["setup"]["score_gap"] > 1e-9, (key, c["setup"]["score_gap"])
        for which, v in c["solves"].items():
            if key[0] != "failing":  # (its one block has no finite residual)
                assert P.huber_margin(v["p"], structure_only=not which) > 1e-6, (key, which)
    # residuals on both sides of the threshold
    v = cases[("n15", 0)]["solves"][1]
    e = P.to_relaxg(v["p"])
    from oracle import pyoracle

    raw = pyoracle.relaxg_eval(e, raw=True)
    sq = np.bincount(raw["row_blk"], weights=raw["r"] ** 2)[:len(v["p"]["blk_cam_a"])]
    assert (sq > F.HUBER_A ** 2).any() and (sq < F.HUBER_A ** 2).any()


def test_the_tie_scene_ties_and_the_others_keep_every_match(cases):
    s = F.tie()
    arr = s.arrays()
    su = F.setup_numpy(arr, _rays(arr), s.cam_q, 4)
    assert su["score_gap"] == 0.0
    assert F.setup_numpy(arr, _rays(arr), s.cam_q, 3)["score_gap"] > 1e-9
    for (name, i), c in cases.items():
        if name == "rough":  # (a match 120 pixels off may score 0: its rays pass each other behind a camera)
            continue
        edges = c["arr"]["edges"]
        for e, l in enumerate(c["setup"]["blk_idx"]):
            live = e < SCENES[name].steps[i]["n_filter"] and c["arr"]["inliers"]["descriptor_score"][int(edges[e]["inlier_offset"])] > 0
            assert len(l) == (int(edges[e]["n_inliers"]) if live else 0), (name, i, e)


def test_the_failing_block_fails_in_the_oracle(cases, oracle):
    v = cases[("failing", 0)]["solves"]
    assert v[0]["ref"]["fail"] and v[1]["ref"]["fail"] and v[1]["d"]["fail"]


@pytest.mark.parametrize("name,i", [k for k in STEPS if k[0] != "failing"])
def test_fp64_evaluation_is_inside_half_of_the_bounds(cases, name, i):
    for which, v in cases[(name, i)]["solves"].items():
        assert not v["ref"]["fail"]
        A, g = _chain_order(v["d"], v["perm"])
        r = F.eval_ratios(v["d"]["cost_reduced"], A, g, v["ref"], v["perm"])
        assert max(r.values()) <= 0.5, (name, i, which, r)


def _first_solve(v, radius=1.0):
    A, g = _chain_order(v["d"], v["perm"])
    scale = F.jacobi_scale(np.diag(A))
    diagonal = F.clamp_diagonal(np.diag(A) * scale * scale)
    lm = F.damping(diagonal, radius)
    return A, g, scale, lm, F.system(A, g, scale, lm)


@pytest.mark.parametrize("name,i", [k for k in STEPS if k[0] != "failing"])
def test_fp64_solve_is_inside_half_of_the_bounds(cases, name, i):
    import scipy.linalg as sl

    for which, v in cases[(name, i)]["solves"].items():
        A, g, scale, lm, W = _first_solve(v)
        n = len(g)
        if n <= F.N_SMALL:
            x, bad = F.small_cholesky(W)
            assert not bad
            r = F.solve_ratios(W, x, 0.5 * np.sum(x * W[n] + lm * x * x), lm)
        else:
            L = np.linalg.cholesky(LM.full(W))
            y = sl.solve_triangular(L, W[n], lower=True)
            x = sl.solve_triangular(L.T, y, lower=False)
            r = F.solve_ratios(W, x, 0.5 * np.sum(x * W[n] + lm * x * x), lm, np.vstack([L, y]))
            assert {"factor", "forward"} <= set(r)
        assert max(r.values()) <= 0.5, (name, i, which, r)
        # the candidate: lm_quat_plus in fp64 against long double, 32 u per component
        q, z = cases[(name, i)]["q"], np.full(3, F.Z0)
        ql, zl = F.candidate_ld(np.nan_to_num(q), z, v["cam_t"], v["n_active"], v["nz"], scale, x)
        q64 =np.array([F.qmul(*_plus64(q[c], scale, x, tc)) if tc >= 0 else q[c] for c, tc in enumerate(v["cam_t"])])
        ok = np.abs(np.nan_to_num(q64) - ql.astype(np.float64)) <= 0.5 * F.C_QUAT * F.U
        assert ok.all(), (name, i, which)


def _plus64(q, scale, x, tc):
    d = -(x[tc:tc + 3] * scale[tc:tc + 3])
    nrm = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    s = np.sin(nrm) / nrm
    return np.array([s * d[0], s * d[1], s * d[2], np.cos(nrm)]), q


# ---- every comparison notices a value a few bound-widths off ----------------------------------------------------------------
CASE = ("n66", 0)


def _eval_case(cases):
    v = cases[CASE]["solves"][1]
    A, g = _chain_order(v["d"], v["perm"])
    return v, A, g, G.bounds(dict(v["ref"], cost=v["ref"]["cost_reduced"]))


def test_one_wrong_entry_of_the_normal_equations_is_noticed(cases):
    v, A, g, b = _eval_case(cases)
    Bc = np.zeros_like(A)
    Bc[np.ix_(v["perm"], v["perm"])] = b["JtJ"]
    i, j = 40, 4  # an entry of an off-diagonal pair block that blocks reach
    cand = [(i, j) for i in range(len(g)) for j in range(i) if Bc[i, j] > 0 and i // 3 != j // 3 and i < 3 * v["n_active"]]
    i, j = cand[len(cand) // 2]
    A2 = A.copy()
    A2[i, j] += 4 * Bc[i, j]
    assert F.eval_ratios(v["d"]["cost_reduced"], A2, g, v["ref"], v["perm"])["JtJ"] > 1.0
    # an entry no block reaches must stay exactly 0: any value there is infinitely far out
    zi, zj = next((i, j) for i in range(len(g)) for j in range(i) if Bc[i, j] == 0)
    A3 = A.copy()
    A3[zi, zj] = 1e-300
    assert F.eval_ratios(v["d"]["cost_reduced"], A3, g, v["ref"], v["perm"])["JtJ"] == np.inf


def test_a_transposed_pair_block_is_noticed(cases):
    """the tp > tq branch of phase_asm taken the wrong way: the 3 x 3 block of a camera pair transposed"""
    v, A, g, b = _eval_case(cases)
    worst = 0.0
    for (a, c) in {(int(x), int(y)) for x, y in zip(v["p"]["blk_cam_a"], v["p"]["blk_cam_b"])}:
        ta, tc = sorted((v["cam_t"][a], v["cam_t"][c]))
        if ta < 0:
            continue
        A2 = np.tril(A).copy()
        A2[tc:tc + 3, ta:ta + 3] = A2[tc:tc + 3, ta:ta + 3].T.copy()
        r = F.eval_ratios(v["d"]["cost_reduced"], A2, g, v["ref"], v["perm"])["JtJ"]
        assert r > 1.0, (a, c, r)
        worst = max(worst, r)
    assert worst > 1e3


def test_a_dropped_chunk_is_noticed(cases, oracle):
    """the second chunk (blocks 64 ..) of the 65-block edge left out of the sums"""
    c = cases[("bootstrap", 2)]
    v = c["solves"][1]
    lists = [l.copy() for l in c["setup"]["blk_idx"]]
    assert len(lists[3]) == 65
    lists[3] = lists[3][:64]
    p = F.plane_problem(c["arr"], c["rays"], lists, c["q"], np.full(3, F.Z0), v["cam_t"], c["step"]["cam_prior"], 1)
    d = oracle.relaxg_eval(P.to_relaxg(p), precision=0)
    A, g = _chain_order(d, v["perm"])
    r = F.eval_ratios(d["cost_reduced"], A, g, v["ref"], v["perm"])
    assert min(r.values()) > 1.0, r


def test_a_wrong_factor_entry_and_the_damping_before_the_scaling_are_noticed(cases):
    import scipy.linalg as sl

    v = cases[CASE]["solves"][1]
    A, g, scale, lm, W = _first_solve(v)
    n = len(g)
    L = np.linalg.cholesky(LM.full(W))
    y = sl.solve_triangular(L, W[n], lower=True)
    x = sl.solve_triangular(L.T, y, lower=False)
    mcc = 0.5 * np.sum(x * W[n] + lm * x * x)
    assert max(F.solve_ratios(W, x, mcc, lm, np.vstack([L, y])).values()) <= 0.5
    L2 = L.copy()
    L2[65, 3] += 4 * LM.C_FACTOR * 5 * F.U * np.sqrt(W[65, 65] * W[3, 3]) / abs(L[3, 3])  # four bound-widths in (W - L L')[65, 3]
    assert F.solve_ratios(W, x, mcc, lm, np.vstack([L2, y]))["factor"] > 1.0
    # the damping added to A before the scaling: a different system, its step is not this one's
    Wb = F.system(A + np.diag(lm), g, scale, np.zeros(n))
    Lb = np.linalg.cholesky(LM.full(Wb))
    xb = sl.cho_solve((Lb, True), Wb[n])
    r = F.solve_ratios(W, xb, 0.5 * np.sum(xb * W[n] + lm * xb * xb), lm, np.vstack([Lb, sl.solve_triangular(Lb, Wb[n], lower=True)]))
    assert r["factor"] > 1.0 and r["backward"] > 1.0, r
    # and one step entry a few bound-widths off
    x2 = x.copy()
    x2[7] *= 1 + 1e-9
    assert F.solve_ratios(W, x2, mcc, lm)["backward"] > 1.0
    assert F.model_ratio(W[n], lm, x, mcc * (1 + 1e-11)) > 1.0


def test_the_small_cholesky_transcription_solves_its_system(cases):
    v = cases[("n12", 0)]["solves"][1]
    A, g, scale, lm, W = _first_solve(v)
    x, bad = F.small_cholesky(W)
    assert not bad and len(x) == 12
    assert np.allclose(LM.full(W) @ x, W[12], rtol=1e-10, atol=0)
    Wn = W.copy()
    Wn[3, 3] = -1.0
    assert F.small_cholesky(Wn)[1]


def test_the_rules_transcription_on_known_sequences():
    """lm_trust and the termination rules (relax_lm_rules.hpp) as F.replay restates them"""
    first = dict(cost=1.0, gmax=1.0, fail_bits=0, x_norm=1.0)
    ok = dict(mcc=0.5, chol_fail=0, step_norm=0.1, cand_norm=1.0, cost=0.5, gmax=1.0, fail_bits=0)
    r = F.replay(first, [ok, dict(ok, cost=0.4999999), ])
    assert r["accepted"] == [True, False] and r["termination"] == F.CONVERGENCE_FUNCTION and r["iterations"] == 3
    assert r["radii"] == [1.0, 3.0]  # rho = 1: 1 - (2 rho - 1)^3 = 0 -> the radius grows by 3
    r = F.replay(first, [dict(ok, cost=2.0), dict(ok, cost=3.0), dict(ok, gmax=1e-11)])
    assert r["accepted"] == [False, False, True] and r["radii"] == [1.0, 0.5, 0.125] and r["termination"] == F.CONVERGENCE_GRADIENT
    r = F.replay(first, [dict(ok, chol_fail=1)] * 5)
    assert r["accepted"] == [None] * 5 and r["termination"] == F.FAILURE and r["radii"] == [1.0, 0.5, 0.25, 0.125, 0.0625]
    assert F.replay(first, [dict(ok, step_norm=1e-9)])["termination"] == F.CONVERGENCE_PARAMETER
    assert F.replay(dict(first, gmax=1e-10), [])["iterations"] == 1
    assert F.replay(dict(first, fail_bits=1), [])["termination"] == F.FAILURE
    assert F.replay(first, [dict(ok, fail_bits=2)])["termination"] == F.FAILURE
    assert F.replay(first, [dict(ok, fail_bits=1), dict(ok, gmax=0.0)])["accepted"] == [False, True]  # a failed candidate costs DBL_MAX
