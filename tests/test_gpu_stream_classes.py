"""The extraction's stream class and the tables a context keeps between chunks (csrc/host/extract_features.cpp, csrc/ctx.hip,
akaze_tables_for in csrc/akaze.hip), on the device, in one child process whose record every test here reads.

Stream classes: two surveys of a 3 x 3 grid of 1000 x 750 views from two threads with OCHIP_EXTRACT_CHUNK=2 - the setup of
test_gpu_extract_handover.py - under OCHIP_EXTRACT_PRIORITY=1 (the launch sequences on contexts of their own, streams of the
lowest priority), =0 (root context and first siblings, default priority) and with OCHIP_EXTRACT_STREAMS=1: feature lists and
edges are ==.  The link graph of a 3 x 3 pipeline.run is == under either priority setting.

Table cache: one context extracts 1000 x 750, 808 x 610, 1000 x 750 again, then 1000 x 750 with another max_keypoints - none
of these is downscaled, so the tile order and the descriptor tables are what is kept - and then 2000 x 1500 (downscaled by the
LDS-staged resize), 2022 x 1526 (width no multiple of 4: the general resize) and 2000 x 1500 again, whose INTER_AREA tables are
kept as well.  Every result is == what a context that has extracted nothing before gives for the same views."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (11, 12)
CHILD_SECONDS = 240   # the child takes some ten seconds
# (width, height, max_keypoints) in the order one context sees them
CACHE_STEPS = ((1000, 750, 30000), (808, 610, 30000), (1000, 750, 30000), (1000, 750, 20000),
               (2000, 1500, 30000), (2022, 1526, 30000), (2000, 1500, 30000))


def _features(g):
    nt = g.node_table()
    feats = []
    for i in range(len(g.node_ids)):
        p = g.node_payload(i)
        feats.append((int(nt["features"][i]), int(nt["sparse"][i]), np.asarray(p["loc"]).tobytes(),
                      np.asarray(p["strength"]).tobytes(), np.asarray(p["desc"]).tobytes()))
    return feats


def _edges(g):
    edges = []
    for e in g.edges():
        edges.append((int(e["source"]), int(e["dest"]), int(e["n_matches"]), int(e["n_inliers"]), e["H"].tobytes(),
                      np.asarray(e["f1"]).tobytes(), np.asarray(e["f2"]).tobytes(), np.asarray(e["match_index"]).tobytes(),
                      e["poses"].tobytes()))
    return edges


def _sized(grid, w, h):
    """the grid's cameras with a w x h sensor of the same footprint"""
    import copy

    g = copy.copy(grid)
    g.model = grid.model.copy()
    g.model[[0, 1, 2, 8, 9]] = [0.75 * w, w / 2, h / 2, w, h]
    return g


def _child(out_path):
    import faulthandler
    from concurrent.futures import ThreadPoolExecutor

    faulthandler.dump_traceback_later(CHILD_SECONDS - 30, exit=True)   # a schedule that does not end: every thread's stack, then out

    from opencalibration_amd import capi, host, pipeline, synth

    def setting(priority, streams):
        os.environ["OCHIP_EXTRACT_PRIORITY"] = priority
        if streams is None:
            os.environ.pop("OCHIP_EXTRACT_STREAMS", None)
        else:
            os.environ["OCHIP_EXTRACT_STREAMS"] = streams

    grid = _sized(synth.make_grid(seed=3, rows=3, cols=3, feats=64), 1000, 750)
    start = pipeline.perturbed_orientations(grid, 0.1, 4)
    owner = capi.Context(0)   # renders and owns the views; the surveys run on contexts of their own
    views = [pipeline.synthetic_views(owner, grid, seed=s) for s in SEEDS]
    record = {}

    # ---- two surveys from two threads under each setting
    for name, priority, streams in (("priority1", "1", None), ("priority0", "0", None), ("one_stream", "1", "1")):
        setting(priority, streams)
        ctx = capi.Context(0)

        def survey(k):
            images, shape = views[k]
            g = host.Graph()
            mid = g.add_model(grid.model)
            g.load_link_images(ctx, images, mid, grid.position, start, 30000, device_shape=shape)
            sig = (_features(g), _edges(g))
            g.close()
            return sig

        with ThreadPoolExecutor(2) as pool:
            record[name] = [f.result() for f in [pool.submit(survey, k) for k in range(len(SEEDS))]]
        ctx.close()

    # ---- the link graph of pipeline.run
    for name, priority in (("run1", "1"), ("run0", "0")):
        setting(priority, None)
        ctx = capi.Context(0)
        images, shape = views[0]
        g, res, _ = pipeline.run(ctx, grid, images, shape, start, relax=False)
        record[name] = (int(res["edges"]), _edges(g))
        g.close()
        ctx.close()
    for images, _ in views:
        owner.synth_views_free(images)

    # ---- the table cache: one context through CACHE_STEPS, a fresh context for every step
    setting("1", "1")
    small = synth.make_grid(seed=5, rows=2, cols=2, feats=64)
    shapes = sorted({(w, h) for w, h, _ in CACHE_STEPS})
    sized = {s: pipeline.synthetic_views(owner, _sized(small, *s), seed=21) for s in shapes}

    def lists(ctx, w, h, max_kp):
        images, shape = sized[(w, h)]
        return [(a.tobytes(), b.tobytes(), c.tobytes(), n) for a, b, c, n in
                host.extract_features_batch(ctx, images, max_kp, device_shape=shape)]

    kept = capi.Context(0)
    record["cache"] = []
    for w, h, max_kp in CACHE_STEPS:
        got = lists(kept, w, h, max_kp)
        fresh = capi.Context(0)
        record["cache"].append((got, lists(fresh, w, h, max_kp)))
        fresh.close()
    kept.close()
    for images, _ in sized.values():
        owner.synth_views_free(images)
    owner.close()
    with open(out_path, "wb") as f:
        pickle.dump(record, f)


@pytest.fixture(scope="module")
def record(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stream_classes") / "record.pkl")
    env = dict(os.environ, OCHIP_EXTRACT_CHUNK="2",
               PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    for name in ("OCHIP_EXTRACT_GATE", "OCHIP_EXTRACT_STREAMS", "OCHIP_EXTRACT_HANDOVER", "OCHIP_EXTRACT_PRIORITY"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True,
                       timeout=CHILD_SECONDS)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(out, "rb") as f:
        return pickle.load(f)


def test_feature_lists_do_not_depend_on_the_stream_class(record):
    for k in range(len(SEEDS)):
        feats, edges = record["priority1"][k]
        assert len(feats) == 9 and min(f[0] for f in feats) > 200 and len(edges) >= 16
        assert record["priority1"][k][0] == record["priority0"][k][0]
        assert record["priority1"][k][0] == record["one_stream"][k][0]
        assert record["priority0"][k][0] == record["one_stream"][k][0]
        assert record["priority1"][k][1] == record["priority0"][k][1] == record["one_stream"][k][1]   # (and the edges)
    assert record["priority1"][0] != record["priority1"][1]   # (the surveys are different views)


def test_link_graph_of_a_pipeline_run_does_not_depend_on_the_stream_class(record):
    n1, edges1 = record["run1"]
    n0, edges0 = record["run0"]
    assert n1 == n0 and len(edges1) >= 16
    assert edges1 == edges0


@pytest.mark.parametrize("step", range(len(CACHE_STEPS)))
def test_kept_tables_give_what_a_fresh_context_gives(record, step):
    got, fresh = record["cache"][step]
    assert len(got) == 4 and min(len(loc) // 16 for loc, _, _, _ in got) > 200
    assert got == fresh
    if step and CACHE_STEPS[step][:2] != CACHE_STEPS[step - 1][:2]:
        assert got != record["cache"][step - 1][0]   # (another shape is another result)


if __name__ == "__main__":
    _child(sys.argv[1])
