"""decompose_vote_kernel (csrc/ransac.hip: cv::decomposeHomographyMat by one lane, the cheirality vote by the wavefront, the
poses in std::stable_sort's order; one wavefront per job, four jobs per workgroup) on homographies with a known motion
(tests/decompose_fixtures.py), which the pipeline tests never give it: every branch of the decomposition, the pure-rotation
threshold, negative and extreme scales, singular and non-finite matrices, votes at the 64-lane edges, flags only in the last
chunk, NaN rays, every tie pattern of the four scores.

All families are the jobs of one launch through the seam ochip_debug_decompose_votes, which runs the unchanged kernel on
given homographies.  Bar: the device equals host.decompose (the same csrc/decompose.hpp, built by g++) bit for bit on the
rays the oracle's image_to_3d gives - poses with NaN positions and the signs of zeros, scores, can_decompose, n_inliers; the
bounded motions stay inside the error model; the votes give the exact expected scores and order.  The device being bit-equal
to the host, its ratios are the host's (tests/test_decompose_oracle.py):
DECOMP_RATIOS device {"q": {"ratio": 0.0333, "job": "general364"}, "rank1": {"ratio": 0.32, "job": "general374"}, "R": {"ratio": 0.2, "job": "rotation_yaw90"}, "t": {"ratio": 0.207, "job": "general364"}}"""
import numpy as np
import pytest

import decompose_fixtures as F
from homography_fit_fixtures import UNIT
from opencalibration_amd import capi, host

pytestmark = pytest.mark.gpu

MODEL10 = np.concatenate([UNIT, [4000.0, 3000.0]])


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def all_jobs():
    """dict(name, case, px1, px2, flags): the motions and the degenerate matrices vote with the common rays, all flagged"""
    p1, p2 = F.common_pixels()
    jobs = [dict(name=c["name"], case=c, px1=p1, px2=p2, flags=np.ones(len(p1), np.uint8)) for c in F.motions() + F.degenerate()]
    return jobs + F.votes()


def _pack(jobs):
    """every job one image pair: (counts, xy, models, RANSAC_JOB_DTYPE rows, matches, H, flags)"""
    counts, xy = [], [np.zeros((0, 2))]
    jd = np.zeros(len(jobs), capi.RANSAC_JOB_DTYPE)
    match_rows, flags = [np.zeros(0, capi.RANSAC_MATCH_DTYPE)], [np.zeros(0, np.uint8)]
    off = 0
    for i, j in enumerate(jobs):
        M = len(j["flags"])
        counts += [M, M]
        xy += [j["px1"].reshape(-1, 2), j["px2"].reshape(-1, 2)]
        m = np.zeros(M, capi.RANSAC_MATCH_DTYPE)
        m["k1"] = m["k2"] = np.arange(M)
        match_rows.append(m)
        flags.append(j["flags"])
        jd[i] = (2 * i, 2 * i + 1, M, 0, off, 0)
        off += M
    H = np.array([j["case"]["H"] for j in jobs]).reshape(-1, 9)
    return counts, np.concatenate(xy), np.tile(UNIT, (2 * len(jobs), 1)), jd, np.concatenate(match_rows), H, np.concatenate(flags)


def _launch(ctx, jobs):
    counts, xy, models, jd, matches, H, flags = _pack(jobs)
    ctx.upload_batch(counts, np.zeros((len(xy), 8), np.uint64), xy, models)
    return ctx.debug_decompose_votes(jd, matches, H, flags)


@pytest.fixture(scope="module")
def host_results(oracle):
    """host.decompose of every job on the oracle's rays of its pixels: name -> (can_decompose, poses, n_inliers)"""
    out = {}
    for j in all_jobs():
        f = j["flags"].astype(bool)
        r1 = oracle.image_to_3d(j["px1"], MODEL10) if len(f) else np.zeros((0, 3))
        r2 = oracle.image_to_3d(j["px2"], MODEL10) if len(f) else np.zeros((0, 3))
        with np.errstate(all="ignore"):
            ok, p = host.decompose(j["case"]["H"], r1[f], r2[f])
        out[j["name"]] = (ok, p, int(f.sum()), r1, r2)
    return out


@pytest.fixture(scope="module")
def device_results(ctx):
    jobs = all_jobs()
    return jobs, _launch(ctx, jobs)


def _differences(jobs, dev, host_results):
    bad = []
    for j, d in zip(jobs, dev):
        ok, p, n_inl, _, _ = host_results[j["name"]]
        if not F._same_bits(d["pose"], p):
            bad.append((j["name"], "poses", d["pose"].tolist(), p.tolist()))
        elif bool(d["can_decompose"]) != ok or int(d["n_inliers"]) != n_inl or d["can_decompose"] not in (0, 1):
            bad.append((j["name"], "can_decompose, n_inliers", int(d["can_decompose"]), ok, int(d["n_inliers"]), n_inl))
    return bad


def test_device_equals_host_bit_for_bit(device_results, host_results):
    jobs, dev = device_results
    assert len(dev) == len(jobs) > 600
    bad = _differences(jobs, dev, host_results)
    assert not bad, bad[:5]


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_partial_last_workgroup(ctx, host_results, n):
    """four jobs per workgroup: launches that fill a part of one, one, and one and a part.  The jobs are taken from the votes
    (the last ones: the longest ray lists lie there) and one bounded motion"""
    jobs = (F.votes()[40:40 + n - 1] + all_jobs()[:1])[:n] if n > 1 else F.votes()[44:45]
    dev = _launch(ctx, jobs)
    assert len(dev) == n
    bad = _differences(jobs, dev, host_results)
    assert not bad, bad[:5]


def test_bounded_motions_within_the_bound(device_results):
    jobs, dev = device_results
    bad, worst = [], F.Worst()
    for j, d in zip(jobs, dev):
        c = j["case"]
        if not c.get("bounded") or "mix" in j:
            continue
        if np.isnan(d["pose"][:c["solutions"], :7]).any():
            bad.append((j["name"], "NaN"))
            continue
        problems, r = F.check_poses(c, d["pose"])
        worst.add(j["name"], r)
        if problems or F.check_order(d["pose"]):
            bad.append((j["name"], problems, r))
    print("DECOMP_RATIOS device " + worst.line())
    assert not bad, bad[:10]


def test_votes_scores_and_order(ctx, device_results, host_results):
    """the exact expected scores and order, from the device's own solutions (a launch of the two vote matrices without a
    single flag gives them in the decomposition's order)"""
    jobs, dev = device_results
    cases = {j["case"]["name"]: j["case"] for j in F.votes()}
    bare = [dict(name="bare_" + k, case=c, px1=np.zeros((1, 2)), px2=np.zeros((1, 2)), flags=np.zeros(1, np.uint8)) for k, c in cases.items()]
    sols = {j["case"]["name"]: F.solutions_by_index(d["pose"]) for j, d in zip(bare, _launch(ctx, bare))}
    bad, n = [], 0
    for j, d in zip(jobs, dev):
        if "mix" not in j:
            continue
        n += 1
        _, _, _, r1, r2 = host_results[j["name"]]
        can, rows, _ = F.expected_rows(j["case"]["H"], sols[j["case"]["name"]], r1, r2, j["flags"])
        if bool(d["can_decompose"]) != can or not F._same_bits(d["pose"], rows) or int(d["n_inliers"]) != int(j["flags"].sum()):
            bad.append((j["name"], d["pose"][:, 7].tolist(), rows[:, 7].tolist(), int(d["can_decompose"]), can))
    assert n == len(F.votes()) and not bad, bad[:10]


def test_seam_rejects_what_it_cannot_run(ctx):
    jobs = F.votes()[5:7]
    counts, xy, models, jd, matches, H, flags = _pack(jobs)
    ctx.upload_batch(counts, np.zeros((len(xy), 8), np.uint64), xy, models)
    assert len(ctx.debug_decompose_votes(jd[:0], matches[:0], H[:0], flags[:0])) == 0
    L, h = ctx.L, ctx.h
    out = np.zeros(len(jd), capi.DECOMPOSITION_DTYPE)
    args = [jd.ctypes.data, len(jd), matches.ctypes.data, len(matches), H.ctypes.data, flags.ctypes.data, out.ctypes.data]
    assert L.ochip_debug_decompose_votes(h, *args) == 0
    for k in (0, 2, 4, 5, 6):   # a NULL in the place of each array
        a = list(args)
        a[k] = None
        assert L.ochip_debug_decompose_votes(h, *a) != 0, k
    assert L.ochip_debug_decompose_votes(None, *args) != 0
    for field, value in (("image_1", 4), ("image_2", 1 << 20), ("match_offset", len(matches)), ("n", len(matches) + 1)):
        bad = jd.copy()
        bad[field][1] = value
        with pytest.raises(capi.OchipError):
            ctx.debug_decompose_votes(bad, matches, H, flags)
    far = matches.copy()
    far["k2"][-1] = int(jd["n"][1])   # a keypoint past its image
    with pytest.raises(capi.OchipError):
        ctx.debug_decompose_votes(jd, far, H, flags)
    assert F._same_bits(ctx.debug_decompose_votes(jd, matches, H, flags)["pose"], out["pose"])
