"""The resident bootstrap chain (csrc/relax_chain.hip) phase by phase, through its trace seam (ochip_plane_chain_trace: the
serial part of an instantiation of the kernel that the product never launches writes what it has just computed into a
buffer) on the scenes of tests/chain_fixtures.py:

  rays         phase_init against host.image_to_3d, to the bit;
  set-up       phase_setup / after_setup / the n_filter == 0 shortcut against ochip_plane_setup_* at the traced orientations
               (keep flags, inexact, block lists to the bit) and a numpy restatement (counts, priors, live chunks, cam_t);
  evaluation   EVERY evaluation of every solve (eval_chunk / phase_eval / phase_asm, eval_serial) against the long-double
               oracle within relax_eval_fixtures.bounds (c = 2^18), unreached entries exactly 0, the clamped diagonal to
               the bit;
  solve        every linear solve (the one-thread Cholesky up to 12 unknowns, phase_chol + after_chol above) - scale, damping
               and scaled gradient to the bit, factor / forward solve / step / model cost change within lm_fixtures' bounds
               (constants 4), the step of a well-conditioned system against a long-double solve;
  candidate    the next evaluation's state against lm_quat_plus in long double (32 u per component); a rejected step
               leaves the state to the bit;
  trajectory   a transcription of lm_trust and the termination rules fed with the traced costs reproduces every radius,
               every decision and the result struct's counters;
  identity     traced resident == traced stepped == ochip_plane_chain_run, bit for bit; the hand-over; the refusals.

The references and bounds are checked without a device in tests/test_chain_trace_oracle.py.  The worst error-to-bound
ratios are printed (CHAIN_TRACE_RATIOS)."""
import ctypes
import json

import numpy as np
import pytest

import chain_fixtures as F
import plane_eval_fixtures as P
from opencalibration_amd import capi, host

pytestmark = pytest.mark.gpu

RATIOS = {}  # quantity -> (worst ratio, case)
SCENES = F.scenes()
TERMINATION = {0: F.NO_PARAMETERS, 1: F.CONVERGENCE_GRADIENT, 2: F.CONVERGENCE_PARAMETER, 3: F.CONVERGENCE_FUNCTION,
               4: F.CONVERGENCE_RADIUS, 5: F.NO_CONVERGENCE, 6: F.FAILURE}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nCHAIN_TRACE_RATIOS " + json.dumps({k: [round(v[0], 4), v[1]] for k, v in sorted(RATIOS.items())}))


def _note(ratios, case):
    for k, v in ratios.items():
        if k not in RATIOS or v > RATIOS[k][0]:
            RATIOS[k] = (v, case)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _chain(ctx, arr):
    return capi.PlaneChain(ctx, arr["edges"], arr["inliers"], arr["cam_pos"], arr["cam_q"], arr["cam_optimize"], arr["models10"],
                           arr["grid_fraction"], arr["huber_a"], arr["prior_weight"], arr["steps"])


def _traced(ctx, arr, stepped=False, **kw):
    ch = _chain(ctx, arr)
    try:
        return ch.trace(stepped=stepped, **kw)
    finally:
        ch.close()


def _structure(events):
    """steps: dict(setup, solves: [dict(first: EVAL or None, iterations: [(SOLVE, EVAL)], finish)])"""
    steps = []
    for ev in events:
        k = ev["kind"]
        if k == capi.TR_SETUP:
            steps.append(dict(setup=ev, solves=[]))
        elif k == capi.TR_EVAL and ev["first"]:
            steps[-1]["solves"].append(dict(first=ev, iterations=[], finish=None))
        elif k == capi.TR_SOLVE:
            steps[-1]["solves"][-1]["iterations"].append([ev, None])
        elif k == capi.TR_EVAL:
            steps[-1]["solves"][-1]["iterations"][-1][1] = ev
        else:
            if not steps[-1]["solves"] or steps[-1]["solves"][-1]["finish"] is not None:
                steps[-1]["solves"].append(dict(first=None, iterations=[], finish=None))  # (a solve without unknowns)
            steps[-1]["solves"][-1]["finish"] = ev
    return steps


@pytest.fixture(scope="module")
def traces(ctx):
    """name -> the scene's arrays, its resident traced run and the run's events by step; one run per scene"""
    out = {}
    for name, s in SCENES.items():
        arr = s.arrays()
        t = _traced(ctx, arr)
        assert t["n_events"] == len(t["events"]), (name, t["n_events"], len(t["events"]))  # nothing fell out of the buffer
        assert t["result"]["status"] == 0 and t["result"]["steps_done"] == len(s.steps), (name, t["result"])
        out[name] = dict(arr=arr, run=t, steps=_structure(t["events"]))
        assert len(out[name]["steps"]) == len(s.steps)
    return out


def _all_solves(traces, skip=()):
    for name, tr in traces.items():
        if name in skip:
            continue
        for i, st in enumerate(tr["steps"]):
            for k, so in enumerate(st["solves"]):
                yield f"{name}/s{i}/{k}", tr, st, so


def test_the_scenes_reach_the_routes(traces):
    """the systems sizes and routes the fixtures are built for, as the chain ran them"""
    sizes = {name: [[so["first"]["n"] if so["first"] else 0 for so in st["solves"]] for st in tr["steps"]]
             for name, tr in traces.items()}
    assert sizes["bootstrap"] == [[0, 3], [3, 6], [3, 12], [3, 12]], sizes["bootstrap"]
    for name, n in (("n12", 12), ("n15", 15), ("n63", 63), ("n66", 66), ("n129", 129), ("rough", 15)):
        assert sizes[name] == [[3, n]], (name, sizes[name])
    b = traces["bootstrap"]["steps"]
    assert b[0]["setup"]["n_filter"] == 0 and b[0]["solves"][1]["first"]["nz"] == 0 and len(b[0]["solves"][1]["iterations"]) >= 2
    assert list(b[1]["setup"]["blk_cnt"]) == [1, 63, 64, 65, 130, 7, 0, 9, 6, 0]
    for name, tr in traces.items():
        for st in tr["steps"]:
            for so in st["solves"]:
                for sv, _ in so["iterations"]:
                    assert sv["tiles"] == (sv["n"] > F.N_SMALL) and sv["chol_fail"] == 0
    states = [so["first"]["state"] for st in b for so in st["solves"] if so["first"]]
    assert set(states) == {0, 1}  # the state buffers alternated across the steps


def test_rays_equal_the_host_to_the_bit(traces):
    for name, tr in traces.items():
        inl = tr["arr"]["inliers"]
        exp = np.concatenate([host.image_to_3d(inl["px1"], F.MODEL10), host.image_to_3d(inl["px2"], F.MODEL10)], 1)
        assert np.array_equal(tr["run"]["rays"], exp), name


def test_setup_equals_the_setup_entries_and_its_restatement(ctx, traces):
    for name, tr in traces.items():
        arr, rays = tr["arr"], tr["run"]["rays"]
        edges = arr["edges"]
        for i, st in enumerate(tr["steps"]):
            ev = st["setup"]
            step = arr["steps"][i]
            assert (ev["step"], ev["mode"], ev["n_filter"], ev["complete"]) == (i, step["mode"], step["n_filter"], 1)
            assert np.array_equal(ev["plane_xy"], step["tri_xy"]) and np.all(ev["z"] == step["z0"])
            nf = ev["n_filter"]
            lists = ev["blk_idx"]
            if nf:
                q = np.where(np.isnan(ev["q"]), 0.0, ev["q"])  # (a camera without an orientation is on no edge in front of n_filter)
                dev = ctx.plane_setup(edges[:nf], arr["inliers"], arr["cam_pos"], q, arr["models10"], ev["plane_xy"], F.GRID)
                mine = np.zeros(len(arr["inliers"]), bool)
                for e in edges[:nf]:
                    mine[int(e["inlier_offset"]):int(e["inlier_offset"]) + int(e["n_inliers"])] = True
                assert np.array_equal(ev["keep"][mine], dev["keep"][mine]), (name, i)
                assert not ev["inexact"].any() and not dev["inexact"].any()
                a = np.concatenate([np.full(len(lists[e]), edges[e]["cam_a"]) for e in range(nf)])
                b = np.concatenate([np.full(len(lists[e]), edges[e]["cam_b"]) for e in range(nf)])
                r = np.concatenate([rays[int(edges[e]["inlier_offset"]) + lists[e]] for e in range(nf)])
                assert np.array_equal(a, dev["blk_cam_a"]) and np.array_equal(b, dev["blk_cam_b"]), (name, i)
                assert np.array_equal(r, dev["blk_rays"]), (name, i)
                su = F.setup_numpy(arr, rays, ev["q"], nf, ev["plane_xy"])
                assert su["score_gap"] > 1e-9
                assert all(np.array_equal(x, y) for x, y in zip(su["blk_idx"], lists)), (name, i)
            assert all(len(lists[e]) == 0 and ev["blk_cnt"][e] == 0 for e in range(nf, len(edges)))
            sn = F.step_numpy(arr, step, ev["q"], lists)
            for k in ("n_blocks", "n_prior", "n_live"):
                assert ev[k] == sn[k], (name, i, k, ev[k], sn[k])
            assert np.array_equal(ev["cam_prior"], sn["cam_prior"]) and np.array_equal(ev["cam_blocks"], sn["cam_blocks"])
            for so in st["solves"]:
                for e in [so["first"]] + [x[1] for x in so["iterations"]]:
                    if e is not None:
                        exp = sn["cam_t"] if e["which"] else np.full(len(sn["cam_t"]), -1)
                        assert np.array_equal(e["cam_t"], exp), (name, i)
                        assert e["n_active"] == (exp >= 0).sum() and e["nz"] == (3 if sn["n_blocks"] else 0)
                        assert e["n"] == 3 * e["n_active"] + e["nz"]


def test_every_evaluation_against_long_double(traces, oracle):
    checked = 0
    for case, tr, st, so in _all_solves(traces, skip=("failing",)):
        if so["first"] is None:
            continue
        arr, rays, lists = tr["arr"], tr["run"]["rays"], st["setup"]["blk_idx"]
        scale = None
        for k, ev in enumerate([so["first"]] + [x[1] for x in so["iterations"]]):
            p = F.plane_problem(arr, rays, lists, ev["q"], ev["z"], ev["cam_t"], st["setup"]["cam_prior"], ev["which"],
                                st["setup"]["plane_xy"])
            ref = oracle.relaxg_eval(P.to_relaxg(p), precision=1, structure_only=not ev["which"])
            assert not ref["fail"] and ev["fail_bits"] == 0 and ref["n"] == ev["n"], (case, k)
            assert P.huber_margin(p, structure_only=not ev["which"]) > 1e-6, (case, k)
            perm = F.columns(ref["order"], ev["cam_t"], ev["n_active"], ev["nz"], ref["n"])
            r = F.eval_ratios(ev["cost"], ev["A"], ev["g"], ref, perm)  # (an entry nothing reaches: bound 0, any value is inf)
            _note(r, f"{case}/e{k}")
            assert max(r.values()) <= 1.0, (case, k, r)
            d = np.diag(ev["A"])
            if k == 0:
                scale = F.jacobi_scale(d)
            assert ev["has_diag"] and np.array_equal(ev["diagonal"], F.clamp_diagonal(d * scale * scale)), (case, k)
            checked += 1
    assert checked > 30, checked


def _current(so, sv):
    """the evaluation whose state a linear solve starts from"""
    for ev in reversed([so["first"]] + [x[1] for x in so["iterations"] if x[1] is not None and x[1]["index"] < sv["index"]]):
        if np.array_equal(ev["q"], sv["q"], equal_nan=True) and np.array_equal(ev["z"], sv["z"]):
            return ev
    raise AssertionError("a linear solve from a state no evaluation saw")


def test_every_linear_solve(traces):
    checked = {0: 0, 1: 0}
    for case, tr, st, so in _all_solves(traces):
        if not so["iterations"]:
            continue
        scale = F.jacobi_scale(np.diag(so["first"]["A"]))
        for k, (sv, _) in enumerate(so["iterations"]):
            cur = _current(so, sv)
            assert np.array_equal(sv["scale"], scale), (case, k)
            lm = F.damping(cur["diagonal"], sv["radius"])
            assert np.array_equal(sv["lm_diag"], lm) and np.array_equal(sv["gs"], cur["g"] * scale), (case, k)
            W = F.system(cur["A"], cur["g"], scale, lm)
            r = F.solve_ratios(W, sv["x"], sv["mcc"], lm, sv.get("L"))
            assert ("factor" in r) == (sv["n"] > F.N_SMALL)
            _note(r, f"{case}/i{k}")
            assert max(r.values()) <= 1.0, (case, k, r)
            checked[sv["tiles"]] += 1
    assert checked[0] > 10 and checked[1] >= 8, checked
    assert "forward_error" in RATIOS


def test_candidates_and_rejected_steps(traces):
    accepted = rejected = 0
    for case, tr, st, so in _all_solves(traces, skip=("failing",)):
        its = so["iterations"]
        for k, (sv, ev) in enumerate(its):
            cur = _current(so, sv)
            ql, zl = F.candidate_ld(np.nan_to_num(sv["q"]), sv["z"], cur["cam_t"], sv["n_active"], sv["nz"], sv["scale"], sv["x"])
            eq = np.abs(np.nan_to_num(ev["q"]) - ql.astype(np.float64)) / (F.C_QUAT * F.U)
            ez = np.abs(ev["z"] - zl.astype(np.float64)) / (F.C_QUAT * F.U * np.maximum(1.0, np.abs(zl.astype(np.float64))))
            r = dict(candidate=float(max(eq.max(), ez.max())))
            _note(r, f"{case}/i{k}")
            assert r["candidate"] <= 1.0, (case, k, r)
            assert np.array_equal(np.isnan(ev["q"]), np.isnan(sv["q"]))
            idle = cur["cam_t"] < 0
            assert np.array_equal(ev["q"][idle], sv["q"][idle], equal_nan=True)  # cameras without unknowns are copied
            if k + 1 < len(its):
                nxt = its[k + 1][0]
                same = np.array_equal(nxt["q"], sv["q"], equal_nan=True) and np.array_equal(nxt["z"], sv["z"])
                took = np.array_equal(nxt["q"], ev["q"], equal_nan=True) and np.array_equal(nxt["z"], ev["z"])
                assert same != took, (case, k)  # the old state to the bit, or the candidate to the bit
                accepted += took
                rejected += same
    assert accepted > 10 and rejected >= 1, (accepted, rejected)  # (the rejections: the scene "rough")
    print(f"\nchain trace: {accepted} accepted and {rejected} rejected steps followed by another")


def test_trajectories_follow_the_rules(traces):
    for name, tr in traces.items():
        finishes = []
        for i, st in enumerate(tr["steps"]):
            for k, so in enumerate(st["solves"]):
                fin = so["finish"]
                assert fin is not None, (name, i, k)
                finishes.append(fin)
                if so["first"] is None:
                    assert TERMINATION[fin["termination"]] == F.NO_PARAMETERS and fin["iterations"] == 0
                    continue
                f = so["first"]
                its = so["iterations"]
                first = dict(cost=f["cost"], gmax=float(np.max(np.abs(f["g"]))), fail_bits=f["fail_bits"],
                             x_norm=its[0][0]["x_norm"] if its else 0.0)
                seq = [dict(mcc=sv["mcc"], chol_fail=sv["chol_fail"], step_norm=np.sqrt(sv["step_norm2"]),
                            cand_norm=np.sqrt(sv["cand_norm2"]), cost=ev["cost"], gmax=float(np.max(np.abs(ev["g"]))),
                            fail_bits=ev["fail_bits"]) for sv, ev in its]
                rep = F.replay(first, seq)
                assert rep["used"] == len(its), (name, i, k, rep["used"], len(its))
                assert rep["radii"] == [sv["radius"] for sv, _ in its], (name, i, k)
                assert rep["termination"] == TERMINATION[fin["termination"]], (name, i, k, rep["termination"], fin)
                assert rep["iterations"] == fin["iterations"], (name, i, k)
                assert fin["initial_cost"] == (0.0 if f["fail_bits"] else f["cost"])
                for j, (sv, ev) in enumerate(its[:-1]):
                    took = np.array_equal(its[j + 1][0]["q"], ev["q"], equal_nan=True) and np.array_equal(its[j + 1][0]["z"], ev["z"])
                    assert took == bool(rep["accepted"][j]), (name, i, k, j)
                assert fin["successful"] == sum(1 for a in rep["accepted"] if a)
        res = tr["run"]["result"]
        assert res["solves"] == len(finishes) and res["iterations_total"] == sum(f["iterations"] for f in finishes), (name, res)
        assert res["last_iterations"] == finishes[-1]["iterations"]
        assert res["last_initial_cost"] == finishes[-1]["initial_cost"] and res["last_final_cost"] == finishes[-1]["final_cost"]


def test_the_failing_block_is_reported(traces):
    st = traces["failing"]["steps"][0]
    assert len(st["solves"]) == 2
    for so in st["solves"]:
        assert so["first"]["fail_bits"] & 1 and not so["iterations"]
        assert TERMINATION[so["finish"]["termination"]] == F.FAILURE
    assert traces["failing"]["run"]["result"]["status"] == 0  # a reported outcome of the solve, not of the chain


def _same(a, b):
    ra, rb = a["result"] if isinstance(a, dict) else a[1], b["result"] if isinstance(b, dict) else b[1]
    qa, qb = a["cam_q"] if isinstance(a, dict) else a[0], b["cam_q"] if isinstance(b, dict) else b[0]
    fields = ("steps_done", "status", "solves", "iterations_total", "last_iterations", "last_residual_blocks", "last_initial_cost",
              "last_final_cost", "plane_z")
    return np.array_equal(qa, qb, equal_nan=True) and all(np.array_equal(ra[f], rb[f]) for f in fields)


@pytest.mark.parametrize("name", F.IDENTITY_SCENES)
def test_traced_stepped_and_untraced_runs_are_identical(ctx, traces, name):
    arr, resident = traces[name]["arr"], traces[name]["run"]
    stepped = _traced(ctx, arr, stepped=True)
    ch = _chain(ctx, arr)
    try:
        plain = ch.run()
    finally:
        ch.close()
    assert _same(resident, stepped) and _same(resident, plain), name
    assert resident["n_events"] == stepped["n_events"] and resident["n_words"] == stepped["n_words"]
    for a, b in zip(resident["events"], stepped["events"]):  # and every traced figure along the way
        assert a.keys() == b.keys()
        for k in a:
            if k == "blk_idx":
                assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))
            elif k not in ("keep", "inexact"):  # (bytes the step's filter does not write are not initialised)
                assert np.array_equal(a[k], b[k], equal_nan=True), (name, a["index"], k)


def test_a_tie_hands_the_step_over(ctx):
    s = F.tie()
    arr = s.arrays()
    t = _traced(ctx, arr)
    assert t["result"]["status"] == 1 and t["result"]["steps_done"] == 1, t["result"]
    last = t["events"][-1]
    assert last["kind"] == capi.TR_SETUP and last["step"] == 1 and not last["complete"] and list(last["inexact"]) == [0, 0, 0, 1]
    # the poses before the step are committed: what the chain of step 0 alone leaves
    alone = dict(arr, steps=arr["steps"][:1])
    ch = _chain(ctx, alone)
    try:
        q0, r0 = ch.run()
    finally:
        ch.close()
    assert r0["status"] == 0 and np.array_equal(t["cam_q"], q0)


def test_buffer_capacity_and_refusals(ctx, traces):
    arr, full = traces["n12"]["arr"], traces["n12"]["run"]
    none = _traced(ctx, arr, capacity=0)
    assert none["n_events"] == full["n_events"] and none["n_words"] == 0 and not none["events"] and _same(none, full)
    # a buffer too small for everything: filled as far as whole events fit, every event counted, the chain unchanged
    part = _traced(ctx, arr, capacity=full["n_words"] // 2)
    assert part["n_events"] == full["n_events"] and 0 < len(part["events"]) < full["n_events"] and _same(part, full)
    # a window of events
    win = _traced(ctx, arr, first_event=2, max_events=3)
    assert [e["index"] for e in win["events"]] == [2, 3, 4] and win["n_events"] == full["n_events"]
    L = ctx.L
    ch = _chain(ctx, arr)
    try:
        q, res = np.zeros((len(arr["cam_pos"]), 4)), np.zeros(1, capi.PLANE_CHAIN_RESULT_DTYPE)
        ne, nw = ctypes.c_uint64(0), ctypes.c_uint64(0)
        args = [ch.h, 0, 0, 10, None, 0, ctypes.byref(ne), ctypes.byref(nw), None, q.ctypes.data, res.ctypes.data]
        for drop in (0, 6, 7, 9, 10):
            bad = list(args)
            bad[drop] = None
            assert L.ochip_plane_chain_trace(*bad) == -1, drop  # OCHIP_EINVAL
        bad = list(args)
        bad[5] = 16  # a capacity without a buffer
        assert L.ochip_plane_chain_trace(*bad) == -1
        # nothing was launched: the chain still runs from its first step
        q1, r1 = ch.run()
        assert _same((q1, r1), full)
    finally:
        ch.close()
