"""GPU parity of the whole link stage (match -> rays -> RANSAC -> decompose -> accept) against the
oracle's restatement of the per-pair closure of src/pipeline/link_stage.cpp:75-112, through the host
library (LinkStage::init/get_runners/finalize) and the C ABI underneath.

Bar: bit-exact match lists, inlier sets, homographies and scores; decomposed poses to 1e-9."""
import numpy as np
import pytest

from opencalibration_amd import capi, host, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _oracle_pair(oracle, grid, a, b, subsets):
    la, _, da, _ = grid.image(a)
    lb, _, db, _ = grid.image(b)
    return oracle.link_pair(la, da, subsets[a], lb, db, subsets[b], grid.model, grid.model)


def _check_grid(ctx, oracle, grid, max_pairs=None):
    g = host.Graph.from_synthetic(grid)
    g.link(ctx, keep_debug=True)
    index_of = {nid: i for i, nid in enumerate(g.node_ids)}
    subsets = [oracle.subsample(*grid.image(i)[:2], 40.0, int(grid.num_sparse[i])) for i in range(grid.n_images)]
    dbg = g.link_debug()
    assert len(dbg) > 0
    checked = 0
    expect = {}
    for d in dbg[:max_pairs]:
        a, b = index_of[d["node"]], index_of[d["match_node"]]
        e = _oracle_pair(oracle, grid, a, b, subsets)
        expect[(d["node"], d["match_node"])] = e
        assert np.array_equal(d["i1"], e["i1"]) and np.array_equal(d["i2"], e["i2"]), (a, b)
        assert np.array_equal(d["dist"], e["dist"]), (a, b)
        assert np.array_equal(d["inliers"], e["inliers"]), (a, b, d["iterations"])
        assert d["score"] == e["score"], (a, b)          # bit-exact fp64
        assert d["can_decompose"] == e["can_decompose"]
        assert (d["iterations"], d["improvements"]) == (e["iterations"], e["improvements"]), (a, b)
        checked += 1
    # the graph edges carry the same payloads, in the reference's deterministic order
    edges = g.edges()
    assert len(edges) == len(dbg)
    for ed in edges:
        e = expect.get((ed["source"], ed["dest"]))
        if e is None:
            continue
        assert np.array_equal(ed["H"], e["H"], equal_nan=True)
        assert np.allclose(ed["poses"], e["poses"], rtol=0, atol=1e-9, equal_nan=True)
        assert np.array_equal(ed["poses"][:, 7], e["poses"][:, 7])     # cheirality votes are integers
        if e["accepted"]:
            assert ed["n_matches"] == len(e["i1"]) and ed["n_inliers"] == e["n_inliers"]
            assert np.array_equal(ed["match_index"], np.flatnonzero(e["inliers"]))
        else:
            assert ed["n_matches"] == 0 and ed["n_inliers"] == 0
    return checked


def test_link_stage_parity_small_grid(ctx, oracle):
    grid = synth.make_grid(2, 3, feats=512, seed=21)
    assert _check_grid(ctx, oracle, grid) == 2 * 3 * 5


def test_link_stage_parity_c1(ctx, oracle):
    """BASELINE config C1: 10 images x 2k features."""
    grid = synth.make_grid(**synth.CONFIGS["C1"])
    assert _check_grid(ctx, oracle, grid) == 90


def test_link_stage_with_outliers_and_few_matches(ctx, oracle):
    """Harder inputs: heavy descriptor noise (fewer ratio-test survivors, real outliers) and a pair of
    images that do not overlap at all (few or no matches, RANSAC early-outs, edge not accepted)."""
    grid = synth.make_grid(1, 4, feats=300, seed=5, flips=95, distractor_frac=1.0, along=60.0)
    assert _check_grid(ctx, oracle, grid) == 4 * 3


@pytest.mark.parametrize("kw, min_iterations", [
    (dict(rows=1, cols=3, feats=300, seed=5, mismatch_frac=0.45), 2000),     # ~20 % inliers: thousands of iterations
    (dict(rows=1, cols=3, feats=200, seed=6, mismatch_frac=0.6, along=40.0), 10000),  # 5 inliers: MAX_ITERATIONS, tiny LO systems
    (dict(rows=2, cols=2, feats=1500, seed=8, mismatch_frac=0.35), 250),     # several hundred matches, hundreds of iterations
    # every Hamming distance 0 -> no correspondence has a quality -> uniform sampling instead of PROSAC (ransac.cpp:83-90)
    (dict(rows=1, cols=3, feats=300, seed=9, mismatch_frac=0.4, flips=0, distractor_frac=0.0), 1000),
    (dict(rows=1, cols=2, feats=60, seed=10, mismatch_frac=0.5, flips=0, distractor_frac=0.0, along=55.0), 10000),
])
def test_ransac_with_true_outliers(ctx, oracle, kw, min_iterations):
    """Matches that are wrong geometrically (same descriptor, random pixel): RANSAC runs hundreds to 10 000 iterations,
    which the kernel walks 32 at a time (fast_forward) - iteration and improvement counts, inlier sets, scores and
    homographies must still be the one-at-a-time loop's, bit for bit."""
    grid = synth.make_grid(**kw)
    g = host.Graph.from_synthetic(grid)
    g.link(ctx, keep_debug=True)
    assert min(d["iterations"] for d in g.link_debug()) >= min_iterations
    g.close()
    assert _check_grid(ctx, oracle, grid) == grid.n_images * (grid.n_images - 1)


def test_link_and_relax_with_lens_distortion(ctx, oracle):
    """Radial + tangential distortion: image_to_3d inverts the lens model per keypoint with the restated TinySolver
    (src/distort/distort_keypoints.cpp:68-103) on the device (rays for RANSAC) and on the host (cheirality vote, relax
    rays); same arithmetic as the oracle's, so match lists, inlier sets and scores stay bit-exact, and the relaxed
    orientations stay within 1e-6."""
    grid = synth.make_grid(2, 3, feats=512, seed=33, distortion=(-0.05, 0.01, -0.002, 1e-3, -5e-4))
    assert np.any(grid.model[3:8] != 0)
    assert _check_grid(ctx, oracle, grid) == 2 * 3 * 5
    g = host.Graph.from_synthetic(grid)
    g.link(ctx)
    rng = np.random.default_rng(8)
    axes = rng.normal(size=(grid.n_images, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    start = synth.quat_mul(grid.orientation, np.concatenate([axes * np.sin(0.05), np.full((grid.n_images, 1), np.cos(0.05))], 1))
    g.set_orientations(start)
    got = g.relax_ground_plane(ctx, start)
    exp = oracle.relax_ground_plane(grid.position, start, grid.model, np.arange(grid.n_images), start, g.edges_flat())
    dots = np.abs(np.sum(got["orientation"] * exp["orientation"], axis=1))
    assert np.all(2 * np.arccos(np.clip(dots, 0, 1)) < 1e-6)
    assert int(got["residual_blocks"]) == exp["residual_blocks"] > 0
    g.close()


def _edge_signature(g):
    return [(e["source"], e["dest"], e["n_matches"], e["n_inliers"], e["H"].tobytes(), e["f1"].tobytes(), e["f2"].tobytes(),
             e["poses"].tobytes()) for e in g.edges()]


def _two_view_rays(n, seed):
    """n points in front of two cameras a small rotation and a baseline apart, as unit rays: n x 6"""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(-2, 2, (n, 2)), rng.uniform(4, 9, (n, 1))], 1)
    c, s = np.cos(0.1), np.sin(0.1)
    Y = (X - (0.7, 0.1, 0.0)) @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).T
    return np.concatenate([X / np.linalg.norm(X, axis=1, keepdims=True), Y / np.linalg.norm(Y, axis=1, keepdims=True)], 1)


def _linked(ctx, grid):
    g = host.Graph.from_synthetic(grid)
    g.link(ctx)
    return g


def _refit(ctx, g, grid):
    new_model = grid.model.copy()
    new_model[0] *= 1.02
    new_model[1] += 7.5
    g.set_model(0, new_model)
    g.refit_edges(ctx)
    return [e["H"].tobytes() for e in g.edges()]


@pytest.mark.parametrize("hooks", ["", "host_sort"])
def test_small_large_small_batches_on_one_context(monkeypatch, hooks):
    """The context's device arrays only grow, and growth drops their contents: a small survey, a larger one (every array
    grows), its refit, an epipolar RANSAC (other structs in the RANSAC scratch) and the small survey again on ONE context
    must give what each gives on a context of its own, byte for byte - with the device's sort and PROSAC order
    (ochip_ransac_homography_batch_sorted, ochip_edge_lists) and with the host's (ochip_ransac_homography_batch)."""
    if hooks:
        monkeypatch.setenv("OCHIP_TEST_HOOKS", hooks)
    small, large = synth.make_grid(1, 2, feats=200, seed=3), synth.make_grid(2, 3, feats=512, seed=21)
    rays = _two_view_rays(100, 4)
    expect = []
    for grid in (small, large):
        fresh = capi.Context(0)
        g = _linked(fresh, grid)
        expect.append((_edge_signature(g), _refit(fresh, g, grid)))
        g.close()
        fresh.close()
    fresh = capi.Context(0)
    expect_epipolar = host.ransac_epipolar(fresh, 1, rays)
    fresh.close()
    assert len(expect[0][0]) == 2 and len(expect[1][0]) == 30

    ctx = capi.Context(0)
    g = _linked(ctx, small)
    assert _edge_signature(g) == expect[0][0]
    g.close()
    g = _linked(ctx, large)
    assert _edge_signature(g) == expect[1][0]
    assert _refit(ctx, g, large) == expect[1][1]
    g.close()
    got = host.ransac_epipolar(ctx, 1, rays)
    assert got[0] == expect_epipolar[0] and np.array_equal(got[1], expect_epipolar[1], equal_nan=True)
    assert np.array_equal(got[2], expect_epipolar[2]) and got[3:] == expect_epipolar[3:]
    g = _linked(ctx, small)
    assert _edge_signature(g) == expect[0][0]
    g.close()
    ctx.close()
