"""The plane relax engine's evaluation on the device (ochip_relax_evaluate: relax_pair_eval_kernel with its 64-block trips,
the role columns of a pair, scatter_cam / scatter_pair / relax_reduce_plane_kernel into the tiles of the block envelope,
the renumbering and the dissection of the camera graph, plane_candidate_kernel's quaternion plus: lm_candidate_cams of
relax_lm_rules.hpp) against the long-double
oracle (oracle/relax_eval.cpp) on the problems of tests/plane_eval_fixtures.py: cost (of the reduced program), J'J and J'r
within the normwise bounds of tests/relax_eval_fixtures.py, the same unknowns (this engine has no padding columns: every
unknown belongs to an active camera or a free height), and a failing block reported as a failure on every route.  Every
problem on route 0 (the current state), route 1 (a candidate the way an accepted LM step evaluates it: state buffers
exchanged, second system set) and route 2 (the candidate as state 1 of the plain evaluation); after accepted solve steps;
with the cameras constant and after undoing it.  The worst error-to-bound ratios are printed (PLANE_EVAL_RATIOS)."""
import json

import numpy as np
import pytest

import plane_eval_fixtures as F
import relax_eval_fixtures as G
from opencalibration_amd import capi

pytestmark = pytest.mark.gpu

RATIOS = {}  # quantity -> (worst ratio, case)
EDGES = {"huber_above", "huber_below"}
PROBLEMS = dict(F.cases() + F.big_cases() + [("plane_iterated", F.plane_iterated())])


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nPLANE_EVAL_RATIOS " + json.dumps({k: [round(v[0], 4), v[1]] for k, v in sorted(RATIOS.items())}))


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _perm(p, ref, dev_order, n_dev):
    """device column of every canonical column: cameras (3 each), then the three heights"""
    groups = [3] * len(p["cam_pos"]) + [1] * 3
    perm = np.full(ref["n"], -1)
    for g, size in enumerate(groups):
        co, do = int(ref["order"][g]), int(dev_order[g])
        assert (co >= 0) == (do >= 0), (g, co, do)
        if co >= 0:
            perm[co:co + size] = do + np.arange(size)
    assert np.all(perm >= 0) and np.all(perm < n_dev) and len(set(perm)) == len(perm)
    return perm


def _compare(name, p, out, oracle, delta_dev=None, structure_only=False):
    n = len(out["Jtr"])
    probe = oracle.relaxg_eval(F.to_relaxg(p, out["cam_q"], out["plane_z"]), precision=0, raw=True,
                               structure_only=structure_only)
    perm = _perm(p, probe, out["order"], n)
    assert n == probe["n"] == out["layout"][0], (name, n, probe["n"], out["layout"])
    delta = None if delta_dev is None else np.asarray(delta_dev)[perm]
    scene = F.to_relaxg(p, out["cam_q"], out["plane_z"])
    ref = oracle.relaxg_eval(scene, precision=1, delta=delta, structure_only=structure_only)
    assert not ref["fail"]
    margin = F.huber_margin(p, delta, structure_only, out["cam_q"], out["plane_z"])
    assert margin >= (0.5e-5 if name.split("/")[0] in EDGES else 1e-6), (name, margin)
    got = dict(cost=out["cost"], JtJ=out["JtJ"][np.ix_(perm, perm)], Jtr=out["Jtr"][perm])
    r = G.ratios(got, F.reduced(ref))
    for k, v in r.items():
        if k not in RATIOS or v > RATIOS[k][0]:
            RATIOS[k] = (v, name)
    assert max(r.values()) <= 1.0, (name, r)
    return r


def _delta(n, seed):
    return np.random.default_rng(seed).normal(size=n) * 1e-3


@pytest.mark.parametrize("route", [0, 1, 2])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_routes_against_long_double(ctx, oracle, name, route):
    p = PROBLEMS[name]
    delta = None
    if route:
        n = ctx.relax_evaluate(p)["layout"][0]
        delta = _delta(n, 100 + route)
    out = ctx.relax_evaluate(p, route=route, delta=delta)
    _compare(f"{name}/r{route}", p, out, oracle, delta)


def test_layouts_are_the_ones_built_for(ctx):
    """n % 64 == 0 and != 0, the renumbering (> 42 active cameras) and the dissection (>= 256: regions and separators)"""
    lay = {name: ctx.relax_evaluate(p) for name, p in PROBLEMS.items()}
    assert lay["n64"]["layout"][0] == 64 and lay["renumbered"]["layout"][0] == 192 and lay["plane"]["layout"][0] % 64 != 0
    assert lay["priors_only"]["layout"][0] == 12 and np.all(lay["priors_only"]["order"][-3:] == -1)
    t = lay["renumbered"]["order"][:-3]
    assert np.any(np.diff(t) < 0)  # not in camera order
    assert lay["renumbered"]["layout"][2] == 1
    n, tail, regions, seps = lay["dissected"]["layout"]
    assert n == 771 and regions >= 2 and seps > 0, lay["dissected"]["layout"]
    # independently of how layout_out counts: the grid is connected, and the cameras in front of the tail, linked among
    # themselves only, fall apart into at least `regions` pieces - the separators (columns >= tail) are what cut it
    p = PROBLEMS["dissected"]
    t = lay["dissected"]["order"][:-3]
    assert np.all(t >= 0) and np.sum(t >= tail) == seps
    assert _components(256, p["blk_cam_a"], p["blk_cam_b"]) == 1
    band = t < tail
    keep = band[p["blk_cam_a"]] & band[p["blk_cam_b"]]
    assert _components(256, p["blk_cam_a"][keep], p["blk_cam_b"][keep], band) >= regions


def _components(n, a, b, members=None):
    """connected components of the camera graph with links (a, b) over the cameras in `members` (all by default)"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for x, y in zip(a, b):
        parent[find(int(x))] = find(int(y))
    members = np.ones(n, bool) if members is None else members
    return len({find(i) for i in range(n) if members[i]})


@pytest.mark.parametrize("name,iterations", [("plane_iterated", 1), ("plane_iterated", 2), ("renumbered", 1),
                                             ("renumbered", 2), ("renumbered", 3)])
def test_after_solve_iterations(ctx, oracle, name, iterations):
    """the state (and its buffers: every accepted step exchanges them, so after an odd number of them the current state
    lives in the second buffers) after the solve's own steps.  plane_iterated: no camera held by its prior alone, which
    the solve turns to where fp64 itself leaves the bound; after its third step the fp64 evaluation itself is at 1.7 of
    the J'r bound (tests/test_plane_eval_oracle.py, test_jtr_bound_after_three_steps_is_broken_by_fp64_itself), so it
    stops at 2."""
    p = PROBLEMS[name]
    out = ctx.relax_evaluate(p, iterations=iterations)
    # every step of these solves is accepted: 1 and 3 leave the state in the exchanged buffers
    assert out["summary"]["successful_steps"] == iterations, out["summary"]
    _compare(f"{name}/it{iterations}", p, out, oracle)
    n = len(out["Jtr"])
    out1 = ctx.relax_evaluate(p, route=1, delta=_delta(n, 7), iterations=iterations)
    _compare(f"{name}/it{iterations}/r1", p, out1, oracle, _delta(n, 7))


@pytest.mark.parametrize("name", ["plane", "renumbered", "dissected"])
def test_cameras_constant_and_undone(ctx, oracle, name):
    p = PROBLEMS[name]
    out = ctx.relax_evaluate(p, cameras_constant=True)
    assert np.all(out["order"][:-3] == -1)
    _compare(f"{name}/constant", p, out, oracle, structure_only=True)
    _compare(f"{name}/undone", p, out["undone"], oracle)


@pytest.mark.parametrize("route", [0, 1, 2])
def test_failing_block_is_reported(ctx, oracle, route):
    """by the evaluation with the Jacobian, on every route (the candidate: delta zero)"""
    p = F.failing()
    assert oracle.relaxg_eval(F.to_relaxg(p))["fail"]
    with pytest.raises(capi.OchipError, match="ochip_relax_evaluate = 1"):
        ctx.relax_evaluate(p, route=route, delta=None if route == 0 else np.zeros(12))
