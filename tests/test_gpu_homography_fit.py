"""The three homography factorisations of the link stage on the device (csrc/homography_fit.hpp: the wave-cooperative 9 x 9
full_piv_lu_solve9, the regenerating regen_lu_solve9 of the tall system, the fast-forward's lane_fit) at the edges the
pipeline tests never reach - inlier counts at the 64-lane edges and below five, flags in the last chunks, sibling pivot
rows, exact ties, rank-deficient and out-of-range systems, NaN coordinates (tests/homography_fit_fixtures.py).

fitInliers + evaluate run through ochip_refit_homography_batch with one round on caller-given flags, every family as the
jobs of one launch; the minimal-sample fits through the seam ochip_debug_homography_fit4.  Bar: bit equality with the
oracle (H, H^-1, flags, inlier count, score, degeneracy; the position of every NaN and the sign of every infinity), and for
the bounded jobs the long-double bounds of the fixtures, which the fp64 oracle keeps with a factor 2 to spare
(tests/test_homography_fit_oracle.py)."""
import json

import numpy as np
import pytest

import homography_fit_fixtures as F
from opencalibration_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _same_bits(a, b):
    """equal values with NaN == NaN, and the same sign wherever the value is not a NaN (the sign of every infinity, of
    every zero)"""
    a, b = np.asarray(a), np.asarray(b)
    ok = ~np.isnan(a)
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a[ok]), np.signbit(b[ok]))


def _launch(ctx, jobs, rounds):
    """every job one image pair of one ochip_refit_homography_batch launch: (H [3, 3], score, n_inliers, flags) per job"""
    counts, xy, models, match_rows, flags = [], [], [], [], []
    jd = np.zeros(len(jobs), capi.RANSAC_JOB_DTYPE)
    off = 0
    for i, j in enumerate(jobs):
        M = len(j["flags"])
        counts += [M, M]
        xy += [j["px1"], j["px2"]]
        models += [j["model1"], j["model2"]]
        m = np.zeros(M, capi.RANSAC_MATCH_DTYPE)
        m["k1"] = m["k2"] = np.arange(M)
        match_rows.append(m)
        flags.append(j["flags"])
        jd[i] = (2 * i, 2 * i + 1, M, 0, off, 0)
        off += M
    xy = np.concatenate(xy)
    ctx.upload_batch(counts, np.zeros((len(xy), 8), np.uint64), xy, np.array(models))
    res, out = ctx.refit_homography(jd, np.concatenate(match_rows), np.concatenate(flags), rounds, F.THR)
    return [(res["H"][i].reshape(3, 3), float(res["score"][i]), int(res["n_inliers"][i]),
             out[int(jd["match_offset"][i]):int(jd["match_offset"][i]) + int(jd["n"][i])]) for i in range(len(jobs))]


def _oracle_rays(oracle, j):
    """the oracle's image_to_3d of the job's pixels (the route tests/test_gpu_refit.py holds bit-equal to the device's)"""
    if len(j["flags"]) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3))
    ext = lambda m: np.concatenate([m, [4000.0, 3000.0]])
    return oracle.image_to_3d(j["px1"], ext(j["model1"])), oracle.image_to_3d(j["px2"], ext(j["model2"]))


class Worst:
    """the worst error-to-bound ratio per quantity and where it came from"""

    def __init__(self):
        self.w = {}

    def add(self, name, r):
        for k in ("H", "Hinv", "score"):
            if k in r and r[k] >= self.w.get(k, (-1.0, ""))[0]:
                self.w[k] = (float(r[k]), name)

    def line(self):
        return json.dumps({k: {"ratio": float("%.3g" % v[0]), "job": v[1]} for k, v in self.w.items()})


def test_fit_inliers_and_evaluate_on_every_family(ctx, oracle):
    jobs = F.all_jobs()
    got = _launch(ctx, jobs, 1)
    bad, worst = [], Worst()
    for j, (H, score, n_inl, flags) in zip(jobs, got):
        p = F.prepared(j)
        r1, r2 = _oracle_rays(oracle, j)
        M = len(r1)
        corr = F.corr7(r1, r2)
        Ho, Hio = oracle.fit_inliers(corr, j["flags"])
        s, inl, err = oracle.evaluate(corr, Ho, Hio)
        if not _same_bits(H, Ho):
            bad.append((j["name"], "H", H.tolist(), Ho.tolist()))
            continue
        if n_inl != int(inl.sum()) or not np.array_equal(flags, inl):
            bad.append((j["name"], "flags", n_inl, int(inl.sum()), np.flatnonzero(flags != inl).tolist()))
        if score != (s / M if M else 0.0):
            bad.append((j["name"], "score", score, s / max(M, 1)))
        if p["bound"]:
            r = F.ratios(H, None, score, flags, p["ref"], p["b"], err=err)
            worst.add(j["name"], r)
            if r["H"] > 1 or r.get("score", 0) > 1 or r.get("flags_off", 0):
                bad.append((j["name"], "bound", r))
    print("HFIT_RATIOS fit_inliers " + worst.line())
    assert not bad, bad


def test_three_rounds_follow_the_oracles_loop(ctx, oracle):
    """rounds = 3 as the re-fit after a model change runs it: every round's fit starts from the previous round's fp64 flags,
    so bit equality is the whole claim"""
    jobs = F.family("scenes") + F.family("few")
    got = _launch(ctx, jobs, 3)
    bad = []
    for j, (H, score, n_inl, flags) in zip(jobs, got):
        r1, r2 = _oracle_rays(oracle, j)
        Ho, inl, so = F.oracle_rounds(oracle, r1, r2, j["flags"], 3)
        if not (_same_bits(H, Ho) and np.array_equal(flags, inl) and n_inl == int(inl.sum()) and score == so):
            bad.append((j["name"], H.tolist(), Ho.tolist(), n_inl, int(inl.sum()), score, so))
    assert not bad, bad


@pytest.fixture(scope="module")
def sample_set(oracle):
    """the specials first, then 2 000 drawn samples: xy16, names, the oracle's fit4 and checkSampleDegeneracy"""
    special = F.special_samples()
    xy = np.concatenate([np.array([s[1] for s in special]), F.samples(2000)])
    names = [s[0] for s in special] + ["drawn%d" % i for i in range(2000)]
    may_bound = [s[2] for s in special] + [True] * 2000
    H, Hi, deg = np.zeros((len(xy), 3, 3)), np.zeros((len(xy), 3, 3)), np.zeros(len(xy), bool)
    one = np.ones((4, 1))
    for i, s in enumerate(xy):
        c = s.reshape(4, 4)
        corr = np.ascontiguousarray(np.concatenate([c[:, :2], one, c[:, 2:], one, 0 * one], 1))
        H[i], Hi[i] = oracle.fit4(corr, [0, 1, 2, 3])
        deg[i] = oracle.check_sample_degeneracy(corr, [0, 1, 2, 3])
    return xy, names, may_bound, H, Hi, deg


@pytest.mark.parametrize("n", [1, 31, 32, 33, None])
def test_minimal_sample_fits_on_both_routes(ctx, sample_set, n):
    """n samples in one call per route (None: all of them): a single one, the partial and full last wavefront of the lane
    route around its 32 samples"""
    xy, names, may_bound, Ho, Hio, dego = sample_set
    n = len(xy) if n is None else n
    out = [ctx.debug_homography_fit4(xy[:n], route) for route in (0, 1)]
    bad, worst = [], Worst()
    for route, (H, Hi, deg) in enumerate(out):
        assert H.shape == (n, 3, 3)
        for i in range(n):
            if not (_same_bits(H[i], Ho[i]) and _same_bits(Hi[i], Hio[i])):
                bad.append((route, names[i], "H", H[i].tolist(), Ho[i].tolist()))
            if deg[i] != dego[i]:
                bad.append((route, names[i], "degenerate", bool(deg[i]), bool(dego[i])))
    for i in range(n):
        if not (_same_bits(out[0][0][i], out[1][0][i]) and _same_bits(out[0][1][i], out[1][1][i])):
            bad.append(("routes differ", names[i]))
    if n == len(xy):
        for i in range(n):
            ref = F.reference_sample(xy[i])
            if not (may_bound[i] and F.sample_bound(ref)):
                continue
            b = F.C_FIT * F.U * ref["kappa"]
            kH = F.kappa_H(ref["H"])
            for route in (0, 1):
                r = dict(H=float(np.max(np.abs(out[route][0][i].astype(F.LD) - ref["H"])) / (b * np.max(np.abs(ref["H"])))))
                if b * kH < F.INVERTIBLE:
                    r["Hinv"] = float(np.max(np.abs(out[route][1][i].astype(F.LD) - ref["Hinv"])) / (b * kH * np.max(np.abs(ref["Hinv"]))))
                worst.add(names[i], r)
                if max(r.values()) > 1:
                    bad.append((route, names[i], "bound", r))
        print("HFIT_RATIOS fit4 " + worst.line())
    assert not bad, bad[:20]


def test_seam_rejects_what_it_cannot_run(ctx):
    H, Hi, deg = ctx.debug_homography_fit4(np.zeros((0, 16)), 0)
    assert H.shape == (0, 3, 3) and len(deg) == 0
    with pytest.raises(capi.OchipError):
        ctx.debug_homography_fit4(np.zeros((1, 16)), 2)
