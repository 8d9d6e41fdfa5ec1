"""Fixtures of the colour-balance tests (tests/test_color_balance_host.py, tests/color_balance_gpu_child.py): synthetic
correspondence sets, the problem file of the oracle driver (tests/color_balance_oracle_driver.cpp), the recorded
yardstick results (tests/golden/color_balance/, scripts/make_color_balance_golden.py), a numpy long-double restatement
of the residuals, Huber's rho and the corrector, and the c u normwise bounds of tests/relax_eval_fixtures.py.

The bounds' constant: the fp64 CPU route's worst error-to-bound ratio with c = 1 over eval_cases() was measured
(MEASURED_RATIO_C1, by test_cpu_evaluation_against_long_double, which prints it); C_BOUND is the next power of two at
or above 8 x that - the margin is for the device's tree-ordered sums."""
import hashlib
import json
import os
import subprocess

import numpy as np

from opencalibration_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "color_balance")
U = 2.0 ** -53
MEASURED_RATIO_C1 = dict(cost=25.97, JtJ=3.155, Jtr=6.869)  # worst over eval_cases(), fp64 CPU route, c = 1
C_BOUND = 2.0 ** 8  # 8 x 25.97 = 207.8 -> 256

# the solve's criteria against the yardstick (the issue's): parameters absolute, final cost relative
PARAM_TOL, COST_RTOL = 1e-6, 1e-9
# solveColorBalance's options (color_balance.cpp:140-148)
FUNCTION_TOL, GRADIENT_TOL, PARAMETER_TOL, MIN_RELATIVE_DECREASE = 1e-4, 1e-6, 1e-4, 1e-3
THRESHOLD_MARGIN = 4.0


def make_corr(n):
    return np.zeros(n, host.CORR_DTYPE)


def scene(pairs, per_pair, cam_model, seed, sigma=10.0, outliers=0.1, ids=None, noise=1.0):
    """Correspondences of a camera graph: `pairs` (a, b) camera indices, per_pair records each (an int or one count per
    pair), camera c has model cam_model[c] and a true Lab offset drawn from N(0, sigma^2); a fraction `outliers` of the
    records is far beyond the Huber scale.  ids: the cameras' node ids (default 1000 + 7 c).  Every second record of a
    pair swaps its sides."""
    rng = np.random.default_rng(seed)
    n_cams = len(cam_model)
    ids = np.array([1000 + 7 * c for c in range(n_cams)] if ids is None else ids, np.uint64)
    off = rng.normal(0, sigma, (n_cams, 3))
    counts = [per_pair] * len(pairs) if isinstance(per_pair, int) else list(per_pair)
    out = []
    for (a, b), k in zip(pairs, counts):
        c = make_corr(k)
        truth = np.stack([rng.uniform(20, 80, k), rng.uniform(-20, 20, k), rng.uniform(-20, 20, k)], 1)
        swap = np.arange(k) % 2 == 1
        ca, cb = np.where(swap, b, a), np.where(swap, a, b)
        bad = rng.random(k) < outliers
        c["lab_a"] = truth + off[ca] + rng.normal(0, noise, (k, 3)) + bad[:, None] * rng.uniform(40, 90, (k, 3))
        c["lab_b"] = truth + off[cb] + rng.normal(0, noise, (k, 3))
        c["camera_id_a"], c["camera_id_b"] = ids[ca], ids[cb]
        c["model_id_a"], c["model_id_b"] = np.asarray(cam_model)[ca], np.asarray(cam_model)[cb]
        for side in "ab":
            c["normalized_radius_" + side] = rng.uniform(0, 1, k)
            c["view_angle_" + side] = rng.uniform(0, 0.5, k)
            c["normalized_x_" + side] = rng.uniform(-0.9, 0.9, k)
            c["normalized_y_" + side] = rng.uniform(-0.9, 0.9, k)
        out.append(c)
    return np.concatenate(out)


def chain_pairs(n, reach=2, first=0):
    return [(first + i, first + i + d) for i in range(n) for d in range(1, reach + 1) if i + d < n]


def grid_pairs(w, h):
    p = []
    for y in range(h):
        for x in range(w):
            if x + 1 < w:
                p.append((y * w + x, y * w + x + 1))
            if y + 1 < h:
                p.append((y * w + x, (y + 1) * w + x))
    return p


def solve_cases():
    """name -> correspondences: the scenes the CPU route, the device route and the recorded yardstick results meet on"""
    cases = {}
    for seed in (1, 2):  # the issue's scene: a 40-camera chain, each camera with the next two, one model
        cases[f"chain40_seed{seed}"] = scene(chain_pairs(40), 200, [3] * 40, seed)
    cases["two_models_mixed"] = scene(chain_pairs(24), 120, [1 if c % 3 else 9 for c in range(24)], 11)
    cases["two_groups"] = scene(chain_pairs(12) + chain_pairs(9, first=12), 150, [2] * 21, 12)
    cases["single_correspondence_camera"] = scene(chain_pairs(10) + [(9, 10)], [100] * len(chain_pairs(10)) + [1], [4] * 11, 15,
                                                   outliers=0.0)
    big = (1 << 63) - 5
    cases["ids_near_2_63"] = scene(chain_pairs(8), 100, [0xFFFFFFF0 + (c % 2) for c in range(8)], 14,
                                   ids=[big - 3 * c for c in range(8)])
    return cases


def grid_case():
    """20 x 20 cameras, 2 403 unknowns: regions and a multi-tile band on the device"""
    return scene(grid_pairs(20, 20), 24, [5] * 400, 21, sigma=5.0)


def nonfinite_case():
    c = scene(chain_pairs(5), 30, [1] * 5, 31)
    c["lab_a"][17, 1] = np.nan
    return c


# ---- the oracle driver ---------------------------------------------------------------------------------------------------
def write_problem(path, corr):
    f32 = lambda v: format(int(np.float32(v).view(np.uint32)), "08x")  # noqa: E731
    with open(path, "w") as f:
        f.write(f"{len(corr)}\n")
        for c in corr:
            vals = [*c["lab_a"], *c["lab_b"], c["normalized_radius_a"], c["normalized_radius_b"], c["view_angle_a"],
                    c["view_angle_b"], c["normalized_x_a"], c["normalized_y_a"], c["normalized_x_b"], c["normalized_y_b"]]
            f.write(f"{int(c['camera_id_a'])} {int(c['camera_id_b'])} {int(c['model_id_a'])} {int(c['model_id_b'])} " +
                    " ".join(f32(v) for v in vals) + "\n")


def build_driver(tmp):
    exe = os.path.join(tmp, "color_balance_oracle_driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-o", exe,
                    os.path.join(ROOT, "tests", "color_balance_oracle_driver.cpp"),
                    os.path.join(ROOT, "oracle", "relax_mini_ceres.cpp")], check=True)
    return exe


def run_driver(exe, corr, tmp, name="problem"):
    path = os.path.join(tmp, name + ".txt")
    write_problem(path, corr)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600, check=True)
    res = dict(iterations=[], per_image={}, per_model={}, checksum=checksum(corr))
    for line in r.stdout.splitlines():
        k, _, rest = line.partition(" ")
        if k == "summary":
            n, usable, c0, c1 = rest.split()
            res.update(num_iterations=int(n), success=bool(int(usable)), initial_cost=float(c0), final_cost=float(c1))
        elif k == "message":
            res["message"] = rest
        elif k == "iteration":
            v = rest.split()
            res["iterations"].append(dict(zip(("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease",
                                               "radius"), map(float, v[:6])), valid=int(v[6]), successful=int(v[7])))
        elif k == "camera":
            v = rest.split()
            res["per_image"][v[0]] = [float(x) for x in v[1:]]
        elif k == "model":
            v = rest.split()
            res["per_model"][v[0]] = [float(x) for x in v[1:]]
    return res


def checksum(corr):
    return hashlib.sha256(np.ascontiguousarray(corr).tobytes()).hexdigest()


def golden(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def thresholds_clear(y):
    """The fixture condition, on the yardstick alone: none of its termination decisions sits within a factor
    THRESHOLD_MARGIN of its threshold.  Returns the list of decisions that do (empty: usable)."""
    its, near, m = y["iterations"], [], THRESHOLD_MARGIN
    norm = float(np.sqrt(sum(v * v for p in list(y["per_image"].values()) + list(y["per_model"].values()) for v in p)))
    cost = its[0]["cost"]
    last = len(its) - 1
    for k, it in enumerate(its):
        if k == 0 or not it["valid"]:
            continue
        ended = k == last and y["message"] != "Maximum number of iterations reached"
        rel = abs(it["cost_change"]) / cost
        if y["message"] == "Function tolerance reached" and k == last:
            # (the oracle leaves the last record's cost empty: the change is relative to the cost before the step)
            if not rel <= FUNCTION_TOL / m:
                near.append(("function tolerance met closely", k, rel))
        elif not rel >= FUNCTION_TOL * m:
            near.append(("function tolerance missed closely", k, rel))
        # the step-norm test: the parameters' norm never exceeds the final one by much on these scenes; 2 x as a cover
        if not it["step_norm"] >= m * PARAMETER_TOL * (2 * norm + PARAMETER_TOL) and not (ended and y["message"] == "Parameter tolerance reached"):
            near.append(("parameter tolerance", k, it["step_norm"], norm))
        if not ended:
            rd = it["relative_decrease"]
            if MIN_RELATIVE_DECREASE / m < rd < MIN_RELATIVE_DECREASE * m:
                near.append(("relative decrease", k, rd))
            if it["successful"]:
                if not it["gradient_max_norm"] >= GRADIENT_TOL * m:
                    near.append(("gradient tolerance", k, it["gradient_max_norm"]))
                cost = it["cost"]
    return near


def compare_solution(got, y, what):
    """the issue's criteria of a route's result `got` (color_balance_solve's dict, before any gauge step: solve without
    positions) against a yardstick result y; returns the worst differences"""
    assert got["success"] == y["success"], (what, got["success"], y["success"])
    assert got["num_iterations"] == y["num_iterations"], (what, got["num_iterations"], y["num_iterations"])
    worst = 0.0
    assert sorted(map(str, got["per_image"])) == sorted(y["per_image"]), what
    for k, v in got["per_image"].items():
        mine = [*v["lab_offset"], v["brdf"], *v["slope"]]
        worst = max(worst, float(np.max(np.abs(np.array(mine) - np.array(y["per_image"][str(k)])))))
    assert sorted(map(str, got["per_model"])) == sorted(y["per_model"]), what
    for k, v in got["per_model"].items():
        worst = max(worst, float(np.max(np.abs(np.array(v) - np.array(y["per_model"][str(k)])))))
    rel = abs(got["final_cost"] - y["final_cost"]) / abs(y["final_cost"])
    print(f"COLOR_BALANCE_DIFF {what}: parameters {worst:.3e} (bound {PARAM_TOL:g}), final cost relative {rel:.3e} "
          f"(bound {COST_RTOL:g}), iterations {got['num_iterations']}")
    assert worst <= PARAM_TOL, (what, worst)
    assert rel <= COST_RTOL, (what, rel)
    return worst, rel


def as_yardstick(res):
    """a route's result in the yardstick's layout (the CPU route as the device's yardstick)"""
    return dict(success=res["success"], num_iterations=res["num_iterations"], final_cost=res["final_cost"],
                per_image={str(k): [*v["lab_offset"], v["brdf"], *v["slope"]] for k, v in res["per_image"].items()},
                per_model={str(k): list(v) for k, v in res["per_model"].items()})


# ---- long-double evaluation -------------------------------------------------------------------------------------------------
def tables(corr):
    cams = np.unique(np.concatenate([corr["camera_id_a"], corr["camera_id_b"]]))
    models = np.unique(np.concatenate([corr["model_id_a"], corr["model_id_b"]]))
    return cams, models


def evaluate_longdouble(corr, cams, models, color6, vig3):
    """cost, J'J, J'r in long double in the canonical order (camera i of `cams` at 6 i, model m at 6 n_cams + 3 m), and
    the block statistics of the bounds.  The functor's float products (r^2, theta^2) are formed in float32 first."""
    L = np.longdouble
    nc, nm, N = len(cams), len(models), len(corr)
    n = 6 * nc + 3 * nm
    x6, v3 = np.asarray(color6, L).reshape(nc, 6), np.asarray(vig3, L).reshape(nm, 3)
    ia, ib = np.searchsorted(cams, corr["camera_id_a"]), np.searchsorted(cams, corr["camera_id_b"])
    ma, mb = np.searchsorted(models, corr["model_id_a"]), np.searchsorted(models, corr["model_id_b"])
    side = {}
    for s, ic, im in (("a", ia, ma), ("b", ib, mb)):
        r2 = (corr["normalized_radius_" + s] * corr["normalized_radius_" + s]).astype(np.float32).astype(L)
        th2 = (corr["view_angle_" + s] * corr["view_angle_" + s]).astype(np.float32).astype(L)
        nx, ny = corr["normalized_x_" + s].astype(L), corr["normalized_y_" + s].astype(L)
        pw = np.stack([r2, r2 * r2, r2 * r2 * r2], 1)
        c = corr["lab_" + s].astype(L) - x6[ic, :3]
        c[:, 0] -= (v3[im] * pw).sum(1) + x6[ic, 3] * th2 + x6[ic, 4] * nx + x6[ic, 5] * ny
        side[s] = dict(c=c, pw=pw, th2=th2, nx=nx, ny=ny)
    r = side["a"]["c"] - side["b"]["c"]  # N x 3
    # local columns: a's camera 0..5, b's camera 6..11, a's model 12..14, b's model 15..17
    J = np.zeros((N, 3, 18), L)
    for s, base, vb, sign in (("a", 0, 12, L(-1)), ("b", 6, 15, L(1))):
        for k in range(3):
            J[:, k, base + k] = sign
        J[:, 0, base + 3] = sign * side[s]["th2"]
        J[:, 0, base + 4] = sign * side[s]["nx"]
        J[:, 0, base + 5] = sign * side[s]["ny"]
        J[:, 0, vb:vb + 3] = sign * side[s]["pw"]
    cols = np.concatenate([6 * ia[:, None] + np.arange(6), 6 * ib[:, None] + np.arange(6), 6 * nc + 3 * ma[:, None] + np.arange(3),
                           6 * nc + 3 * mb[:, None] + np.arange(3)], 1)  # N x 18 (a shared model: columns 12..14 = 15..17)
    sq = (r * r).sum(1)
    a = L(5)
    out = sq > a * a
    root = np.sqrt(np.where(out, sq, L(1)))
    rho0 = np.where(out, 2 * a * root - a * a, sq)
    rho1 = np.where(out, a / root, L(1))
    rho2 = np.where(out, -rho1 / (2 * np.where(out, sq, L(1))), L(0))
    corrected = (sq != 0) & (rho2 > 0)  # (never, under Huber: rho'' <= 0 takes the corrector's plain branch)
    D = 1 + 2 * sq * rho2 / rho1
    alpha = np.where(corrected, 1 - np.sqrt(np.where(corrected, D, L(1))), L(0))
    s1 = np.sqrt(rho1)
    rs = s1 / (1 - alpha)
    asn = np.where(corrected, alpha / np.where(sq != 0, sq, L(1)), L(0))
    rtj = np.einsum("nk,nkc->nc", r, J)
    Jc = s1[:, None, None] * (J - asn[:, None, None] * r[:, :, None] * rtj[:, None, :])
    rc = rs[:, None] * r
    JtJ, Jtr = np.zeros((n, n), L), np.zeros(n, L)
    blockJ = np.einsum("nki,nkj->nij", Jc, Jc)
    np.add.at(JtJ, (cols[:, :, None], cols[:, None, :]), blockJ)
    np.add.at(Jtr, cols, np.einsum("nki,nk->ni", Jc, rc))
    cost = (rho0 / 2).sum()
    # priors: weight 0.1 sqrt(max(1, appearances))
    ccount = np.bincount(np.concatenate([ia, ib]), minlength=nc)
    mcount = np.bincount(np.concatenate([ma, mb]), minlength=nm)
    w = L(0.1) * np.sqrt(np.concatenate([np.repeat(np.maximum(ccount, 1), 6), np.repeat(np.maximum(mcount, 1), 3)]).astype(L))
    x = np.concatenate([x6.ravel(), v3.ravel()])
    JtJ[np.arange(n), np.arange(n)] += w * w
    Jtr += w * (w * x)
    cost += ((w * x) ** 2).sum() / 2
    # block statistics of the bounds (relax_eval_fixtures.bounds): rows_b ||J_b||^2_max over the pairs of columns a
    # block touches, ||J_b||_max ||r_b|| over its columns; a prior is a block of one column per row
    jmax = np.abs(Jc).max((1, 2)).astype(float)
    rn = np.sqrt((rc * rc).sum(1)).astype(float)
    BJ, Bg = np.zeros((n, n)), np.zeros(n)
    touched = np.ones((N, 18), bool)
    np.add.at(BJ, (cols[:, :, None], cols[:, None, :]), (3 * jmax ** 2)[:, None, None] * (touched[:, :, None] & touched[:, None, :]))
    np.add.at(Bg, cols, (jmax * rn)[:, None] * touched)
    wf, xf = w.astype(float), np.abs(x).astype(float)
    BJ[np.arange(n), np.arange(n)] += wf ** 2
    Bg += wf * (wf * xf)
    return dict(cost=cost, JtJ=JtJ, Jtr=Jtr, n=n, BJ=BJ, Bg=Bg, failed=bool(~np.isfinite(r.astype(float)).all()))


def canonical(ev, nc, nm):
    """an evaluation seam's J'J and J'r in the canonical order"""
    perm = np.concatenate([(ev["cam_col"][:, None] + np.arange(6)).ravel(), (ev["model_col"][:, None] + np.arange(3)).ravel()])
    return dict(cost=ev["cost"], JtJ=ev["JtJ"][np.ix_(perm, perm)], Jtr=ev["Jtr"][perm])


def _ratio(err, bound):
    err, bound = np.abs(np.asarray(err, float)), np.asarray(bound, float)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r))


def eval_ratios(got, ref, c=1.0):
    """worst error-to-bound ratios (bounds c u x the block sums) of a canonical evaluation against the long-double one"""
    L = np.longdouble
    return dict(cost=_ratio(float(L(got["cost"]) - ref["cost"]), c * U * float(abs(ref["cost"]))),
                JtJ=_ratio((got["JtJ"].astype(L) - ref["JtJ"]).astype(float), c * U * ref["BJ"]),
                Jtr=_ratio((got["Jtr"].astype(L) - ref["Jtr"]).astype(float), c * U * ref["Bg"]))


def eval_cases():
    """name -> (correspondences, seed of the parameters): states away from 0, so that every term of the residual acts"""
    multi = scene(chain_pairs(30, reach=3), 40, [100 + c for c in range(30)], 41)  # 180 + 90 unknowns: band and tail of several blocks
    return dict(chain=(scene(chain_pairs(12), 60, [3] * 12, 42), 1), mixed_models=(scene(chain_pairs(9), 50, [c % 2 for c in range(9)], 43), 2),
                multi_block_tail_and_band=(multi, 3))


def eval_state(corr, seed):
    cams, models = tables(corr)
    rng = np.random.default_rng(seed)
    return cams, models, rng.normal(0, 3, (len(cams), 6)), rng.normal(0, 2, (len(models), 3))


def smooth_images(n, rows, cols, brighter=(1, 2), offset=25):
    """the same smooth pattern in every image (overlapping samples nearly agree), the `brighter` images offset (of the
    four-camera fixture the two on one diagonal: a pattern the gauge plane cannot absorb)"""
    y, x = np.mgrid[0:rows, 0:cols]
    base = np.stack([110 + 40 * np.sin(x / 23.0) * np.cos(y / 17.0), 120 + 30 * np.cos(x / 31.0), 100 + 35 * np.sin(y / 19.0)], -1)
    return [np.clip(base + (offset if i in brighter else 0), 0, 255).astype(np.uint8) for i in range(n)]


MOSAIC_PLAN = dict(width=105, height=90, gsd=0.1, min_x=-2.0, max_x=8.5, min_y=-2.0, max_y=7.0, mean_camera_z=10.0)
MOSAIC_CONFIG = dict(tile_size=32, blend_transition_radius=10, correspondence_subsample=4)
