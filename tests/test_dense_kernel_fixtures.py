"""The fixtures of tests/dense_kernel_fixtures.py checked on the CPU: the fp64 restatement of dense_predict_kernel and of the
two triangulation kernels agrees with the long-double reference (slot rows, counts and roots exactly; validity exactly and the
points within the bound, which is where C_TRI is calibrated), the margins drop at most 1 %, every family holds the cases it is
named for, and every mutation of the restatement that can be told from the kernel fails at least one family.  No device.

Measured here (fp64 numpy against long double, all 330 tracks): worst error / (2^-53 kappa scale) = 3.73 at "tri2/bulk11";
C_TRI = 2^3 is the next power of two at or above twice that."""
import math

import numpy as np
import pytest

import dense_kernel_fixtures as F


# ------------------------------------------------------------------------------------------------------------ predict
def _predict_by_family():
    out = {}
    for s in F.predict_scenes():
        out.setdefault(s["family"], []).append(s)
    return out


def _predict_problems(s, mutation=None):
    rows, queries, matches, roots = F.predict_fp64(s, mutation)
    bad = []
    if not np.array_equal(rows, s["exp_slot_by_id"]):
        k = int(np.nonzero((rows != s["exp_slot_by_id"]).any(1))[0][0])
        bad.append("%s: slot row of measurement %d is %s, expected %s" % (s["name"], k, rows[k], s["exp_slot_by_id"][k]))
    if (queries, matches) != (s["exp_queries"], s["exp_queries"]):
        bad.append("%s: counts %d %d, expected %d twice" % (s["name"], queries, matches, s["exp_queries"]))
    if not np.array_equal(roots, s["exp_root"]):
        bad.append("%s: roots differ" % s["name"])
    return bad


def test_predict_restatement_agrees_with_the_reference():
    for s in F.predict_scenes():
        assert _predict_problems(s) == []


def test_predict_contents_reach_the_cases_they_are_for():
    fam = _predict_by_family()
    assert set(fam) == {"counts", "far", "distortion", "ties", "clamp"}
    total = 0
    for s in F.predict_scenes():
        f = F.predict_facts(s)
        print("DENSE_PREDICT_SCENE", s["name"], "points", len(s["P"]), "dropped", s["dropped"], {k: v for k, v in f.items() if k != "sources"})
        assert s["dropped"] <= F.DROP_CAP * s["generated"], s["name"]
        assert s["dropped"] == 0 or not s["exact"]
        assert f["features"] >= 300 and len(s["P"]) >= 40, s["name"]
        assert f["no_hit"] >= 10 and f["out_of_image_candidates"] >= 1, s["name"]
        n = s["n_images"]
        assert {0, n // 2, n - 1} <= f["sources"], s["name"]            # both tails of camera_at, and its two-sided part
        assert (s["exp_slot_by_id"][s["nohit"]] == F.NONE).all()
        total += f["features"]
    assert 3000 <= total <= 10000, total
    assert tuple(s["n_images"] for s in fam["counts"]) == F.COUNT_SIZES
    assert {s["n_images"] % 4 for s in fam["counts"]} == {0, 1, 2, 3}
    for s in fam["counts"]:        # 11 cameras: the source is always one of the 11, ten candidates at most
        assert (s["exp_slot_by_id"] != F.NONE).sum(1).max() <= min(s["n_images"] - 1, F.DENSE_K)
    far = F.predict_facts(fam["far"][0])
    assert far["src_outside"] >= 50 and far["full_rows"] >= 50, far       # all 11 slots are candidates
    ties = [F.predict_facts(s) for s in fam["ties"]]
    for size in (2, 3, 4):
        assert sum(t["ties"][size] for t in ties) >= 5, (size, ties)
    assert sum(t["ties_across_rank_11"] for t in ties) >= 3
    assert sum(t["exactly_zero"] for t in ties) >= 3 and sum(t["exactly_cols"] for t in ties) >= 3
    assert all(s["exact"] for s in fam["ties"]) and not any(s["exact"] for f_ in fam for s in fam[f_] if f_ != "ties")
    assert [tuple(s["models"][0, 3:8]) for s in fam["distortion"]] == [F.DIST_A, F.DIST_B]
    clamp = F.predict_facts(fam["clamp"][0])
    assert clamp["clamped_inside"] >= 10 and clamp["clamped_above"] >= 5 and clamp["clamped_outside"] >= 10, clamp


@pytest.mark.parametrize("mutation", F.PREDICT_MUTATIONS)
def test_predict_mutation_is_caught(mutation):
    caught = {fam for fam, scenes in _predict_by_family().items() if any(_predict_problems(s, mutation) for s in scenes)}
    print("DENSE_PREDICT_MUTATION", mutation, sorted(caught))
    assert caught
    expected = {"tie_high": "ties", "gt_cols": "ties", "no_clamp": "clamp", "no_k2": "distortion", "ten_nearest": "far", "keep_source": "counts"}
    assert expected[mutation] in caught


def test_index_layout_is_a_permutation():
    for s in F.predict_scenes():
        ix = F.index_arrays(s["features"])
        assert ix["total"] == s["total"] and sorted(ix["id_of_pos"].tolist()) == list(range(s["total"]))
        hits, rows = F.by_position(s, ix)
        assert np.array_equal(np.isnan(hits[:, 0]), s["nohit"][ix["id_of_pos"]])


# -------------------------------------------------------------------------------------------------------- triangulate
_RUNS = {}


def _tri_run(oracle, mutation=None):
    """per scene the fp64 restatement of every track, once per mutation"""
    if mutation not in _RUNS:
        _RUNS[mutation] = [[F.tri_fp64(s, t, oracle.image_to_3d, mutation) for t in s["tracks"]] for s in F.tri_scenes(oracle.image_to_3d)]
    return _RUNS[mutation]


def _tri_failures(oracle, mutation):
    """family -> the tracks on which the restatement misses the reference"""
    out = {}
    for s, run in zip(F.tri_scenes(oracle.image_to_3d), _tri_run(oracle, mutation)):
        for t, r in zip(s["tracks"], run):
            problem, _ = F.check_track(t, r["valid"], r["point"])
            if problem:
                out.setdefault(t["family"], []).append(problem)
    return out


def test_triangulate_restatement_keeps_the_bound_with_a_factor_two(oracle):
    """the calibration of C_TRI"""
    worst, where, n_valid = 0.0, None, 0
    for s, run in zip(F.tri_scenes(oracle.image_to_3d), _tri_run(oracle)):
        for t, r in zip(s["tracks"], run):
            problem, ratio = F.check_track(t, r["valid"], r["point"], C=math.inf)
            assert problem is None, problem                      # validity, exactly
            assert (r["pair"] == t["ref"]["pair"]) and np.array_equal(r["inliers"], t["ref"]["inliers"]), t["name"]
            if ratio is not None:
                n_valid += 1
                if ratio > worst:
                    worst, where = ratio, t["name"]
    print("DENSE_TRI_CALIBRATION", {"worst_ratio": float("%.3g" % worst), "track": where, "valid_tracks": n_valid, "C_TRI": F.C_TRI})
    assert n_valid >= 250
    assert F.C_TRI == 2.0 ** math.ceil(math.log2(2 * worst)), (worst, where)
    assert _tri_failures(oracle, None) == {}


def test_triangulate_contents_reach_the_cases_they_are_for(oracle):
    scenes = {s["name"]: s for s in F.tri_scenes(oracle.image_to_3d)}
    facts = {k: F.tri_facts(s) for k, s in scenes.items()}
    for k, f in facts.items():
        print("DENSE_TRI_SCENE", k, "features", scenes[k]["total"], f)
    assert sum(len(f["dropped"]) for f in facts.values()) <= F.DROP_CAP * sum(f["generated"] for f in facts.values())
    assert [scenes[k]["cams"]["n"] for k in ("tri2", "tri3", "tri30")] == [2, 3, 30]
    for k in ("tri2", "tri3", "tri30"):
        f = facts[k]
        assert set(F.TRACK_SIZES) <= f["sizes"], k
        assert set(F.SECOND_PAIRS) <= f["pairs_small"] and set(F.SECOND_PAIRS + F.LANE_PAIRS) <= f["pairs_large"], (k, f)
        assert f["few"] >= 4 and f["first_fails"] >= 6 and f["behind_one"] >= 1 and f["repeated_image_in_large"] >= 6, (k, f)
        assert {"sizes", "second", "lanes", "few", "behind", "edge", "bulk"} <= set(f["families"]), k
    for k in ("tri3", "tri30"):
        assert facts[k]["second_fails"] >= 2 and facts[k]["behind_both"] >= 2 and facts[k]["distorted_pairs"] >= 40, (k, facts[k])
    assert not scenes["tri2"]["cams"]["models"][:, 3:8].any() and facts["tri2"]["valid"] >= 50      # rays in long double throughout
    e = facts["exact"]
    assert e["families"] == {"equal": 6, "opposite": 6, "second_fails": 2, "clamp": 2} and e["denom_zero"] == 14 and e["valid"] == 2, e
    # equal and opposite directions: denom is exactly 0 in both precisions, at the first pair or at the second
    for t, r in zip(scenes["exact"]["tracks"], _tri_run(oracle)[3]):
        if t["family"] in ("equal", "opposite"):
            assert r["first"]["denom"] == 0 and t["ref"]["first"]["denom"] == 0, t["name"]
        if t["family"] == "second_fails":
            assert r["second"]["denom"] == 0 and t["ref"]["second"]["denom"] == 0 and t["ref"]["pair"] is None, t["name"]
        if t["family"] == "clamp":      # the member behind its camera is an outlier only because of the clamp
            assert t["ref"]["depth"][2] == 1e-3 and not t["ref"]["inliers"][2] and t["ref"]["valid"], t["name"]
    # every feature of an index is a member of a track: the first and the last position of every image, the last image's too
    for s in scenes.values():
        members = np.concatenate([t["members"] for t in s["tracks"]])
        assert sorted(members.tolist()) == list(range(s["total"])) and all(len(loc) for loc, _ in s["features"]), s["name"]
    # the calls: around the thread kernel's workgroup of 128 and the wavefront kernel's four tracks per workgroup
    s = scenes["tri30"]
    n_large = lambda call: sum(len(s["tracks"][i]["images"]) > F.TRI_LARGE for i in s["calls"][call])
    assert [len(s["calls"][k]) for k in ("empty", "one", "one_large", "first127", "first128", "first129")] == [0, 1, 1, 127, 128, 129]
    assert [n_large(k) for k in ("one", "one_large", "large4", "large5")] == [0, 1, 4, 5]
    assert n_large("large_only") == len(s["calls"]["large_only"]) >= 20 and len(s["calls"]["all"]) == len(s["tracks"]) > 129
    for call in s["calls"]:
        start, member = F.call_arrays(s, s["calls"][call])
        assert len(start) == len(s["calls"][call]) + 1 and start[-1] == len(member)


@pytest.mark.parametrize("mutation", F.TRI_MUTATIONS)
def test_triangulate_mutation_is_caught(oracle, mutation):
    caught = _tri_failures(oracle, mutation)
    print("DENSE_TRI_MUTATION", mutation, {k: len(v) for k, v in caught.items()})
    assert caught
    expected = {"second_from_members": "second", "lane_second": "lanes", "lane_first_only": "lanes", "no_sign_rule": "second_fails",
                "no_clamp": "clamp", "no_k2": "edge", "max_err_wide": "edge", "max_err_narrow": "edge"}
    assert expected[mutation] in caught


@pytest.mark.parametrize("mutation", F.EQUIVALENT_MUTATIONS)
def test_the_equivalent_mutation_is_equivalent(oracle, mutation):
    """`denom > 1e-9` for `|denom| > 1e-9`: no track tells them apart, and none can - over every pair the kernels intersect
    here the fp64 denom stays above -2^-50 n11 n22, seven orders of magnitude from the threshold (see the fixture docstring)"""
    assert _tri_failures(oracle, mutation) == {}
    lowest = 0.0
    for base, mutant in zip(_tri_run(oracle), _tri_run(oracle, mutation)):
        for a, b in zip(base, mutant):
            assert a["valid"] == b["valid"] and (not a["valid"] or np.array_equal(a["point"], b["point"]))
            for I in (a["first"], a["second"]):
                if I is not None:
                    lowest = min(lowest, float(I["denom"] / (I["n11"] * I["n22"])))
    assert lowest >= -2.0 ** -50, lowest
