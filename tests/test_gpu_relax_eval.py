"""The general relax engine's evaluation on the device (ochip_relaxg_evaluate: ray_record_kernel, prior_kernel, the band and
tail assembly with its chunk merges, the cost reduction) against the long-double oracle (oracle/relax_eval.cpp) on the
fixtures of tests/relax_eval_fixtures.py: cost, J'J and J'r within the normwise bounds of that file, the same unknowns, and
a failing block reported as a failure.  The worst error-to-bound ratios are printed (RELAX_EVAL_RATIOS).

The plane engine (relax.hip) is covered the same way by tests/test_gpu_relax_plane_eval.py, and the points engine
(relax_points.hip: its evaluation and its Schur step) by tests/test_gpu_relaxp_eval.py.  The resident chain's copy of the
plane evaluation (relax_chain.hip) is held to the same bounds through its trace seam by tests/test_gpu_chain_trace.py."""
import json

import numpy as np
import pytest

import relax_eval_fixtures as F
from opencalibration_amd import capi

pytestmark = pytest.mark.gpu

RATIOS = {}  # quantity -> (worst ratio, case)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nRELAX_EVAL_RATIOS " + json.dumps({k: [round(v[0], 4), v[1]] for k, v in sorted(RATIOS.items())}))


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _groups(scene):
    """sizes of the unknown groups of an order array: cameras, vertices, f, pp, k"""
    return [3] * len(scene["cam_pos"]) + [1] * len(scene["vert_z"]) + [1, 2, int(scene.get("n_radial_free", 0))]


def _to_canonical(scene, ref, dev_order, n_dev):
    """device column of every canonical column; the groups both sides treat as unknowns must be the same"""
    perm = np.full(ref["n"], -1)
    for g, size in enumerate(_groups(scene)):
        co, do = int(ref["order"][g]), int(dev_order[g])
        assert (co >= 0) == (do >= 0), (g, co, do)
        if co >= 0:
            perm[co:co + size] = do + np.arange(size)
    assert np.all(perm >= 0) and np.all(perm < n_dev) and len(set(perm)) == len(perm)
    return perm


def _check(ctx, oracle, name, scene, structure_only):
    ref = oracle.relaxg_eval(scene, precision=1, structure_only=structure_only)
    assert not ref["fail"]
    cost, JtJ, Jtr, order = ctx.relaxg_evaluate(scene, structure_only=structure_only)
    perm = _to_canonical(scene, ref, order, len(Jtr))
    pad = np.setdiff1d(np.arange(len(Jtr)), perm)  # the padding between regions: unknowns nobody owns
    assert not np.any(JtJ[pad]) and not np.any(JtJ[:, pad]) and not np.any(Jtr[pad]), name
    got = dict(cost=cost, JtJ=JtJ[np.ix_(perm, perm)], Jtr=Jtr[perm])
    r = F.ratios(got, ref)
    for k, v in r.items():
        if k not in RATIOS or v > RATIOS[k][0]:
            RATIOS[k] = (v, name)
    assert max(r.values()) <= 1.0, (name, r)


@pytest.mark.parametrize("name,scene,structure_only", F.cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_evaluation_against_long_double(ctx, oracle, name, scene, structure_only):
    _check(ctx, oracle, name, scene, structure_only)


@pytest.mark.parametrize("name,scene,structure_only", F.big_cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_chunked_owners_against_long_double(ctx, oracle, name, scene, structure_only):
    """band owners past 2 BAND_CHUNK records and tail owners over many chunks: the merges of both"""
    _check(ctx, oracle, name, scene, structure_only)


def test_failing_block_is_reported(ctx, oracle):
    s = F.failing()
    assert oracle.relaxg_eval(s)["fail"]
    with pytest.raises(capi.OchipError):
        ctx.relaxg_evaluate(s)
