"""The hand-over of the extraction contexts between surveys (csrc/host/extract_slots.hpp) on the device: three surveys of
a 3 x 3 grid of 1000 x 750 views from two threads - as bench.py drives them - with OCHIP_EXTRACT_CHUNK=2 (five chunks on four
slots: not a multiple), under OCHIP_EXTRACT_HANDOVER=slot and =survey in child processes.  Feature lists, edges (match
lists - indices into the images' 40 px subsets -, inlier sets, homographies, poses) are == between the two schedules and ==
the same surveys run one after the other in the same child.  One more case gives the middle survey a max_keypoints that is
too small: it fails with its message, and the survey after it completes and equals the reference run."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (11, 12, 13)
CHILD_SECONDS = 180   # a child takes a few seconds


def _signature(g):
    nt = g.node_table()
    feats = []
    for i in range(len(g.node_ids)):
        p = g.node_payload(i)
        feats.append((int(nt["features"][i]), int(nt["sparse"][i]), np.asarray(p["loc"]).tobytes(),
                      np.asarray(p["strength"]).tobytes(), np.asarray(p["desc"]).tobytes()))
    edges = []
    for e in g.edges():
        edges.append((int(e["source"]), int(e["dest"]), int(e["n_matches"]), int(e["n_inliers"]), e["H"].tobytes(),
                      np.asarray(e["f1"]).tobytes(), np.asarray(e["f2"]).tobytes(), np.asarray(e["match_index"]).tobytes(),
                      e["poses"].tobytes()))
    return feats, edges


def _child(out_path, fail_middle):
    """Runs in a child process: the surveys from two threads, then one after the other."""
    import faulthandler
    from concurrent.futures import ThreadPoolExecutor

    faulthandler.dump_traceback_later(CHILD_SECONDS - 30, exit=True)   # a schedule that does not end: every thread's stack, then out

    from opencalibration_amd import capi, host, pipeline, synth

    grid = synth.make_grid(seed=3, rows=3, cols=3, feats=64)
    w, h = 1000, 750
    grid.model = grid.model.copy()
    grid.model[[0, 1, 2, 8, 9]] = [750.0, w / 2, h / 2, w, h]   # the same footprints at a quarter of the resolution
    ctx = capi.Context(0)
    start = pipeline.perturbed_orientations(grid, 0.1, 4)
    views = [pipeline.synthetic_views(ctx, grid, seed=s) for s in SEEDS]

    def survey(k, max_keypoints=30000):
        images, shape = views[k]
        g = host.Graph()
        mid = g.add_model(grid.model)
        try:
            g.load_link_images(ctx, images, mid, grid.position, start, max_keypoints, device_shape=shape)
        except capi.OchipError as ex:
            g.close()
            return ("error", str(ex))
        sig = _signature(g)
        g.close()
        return sig

    kp = [30000, 40 if fail_middle else 30000, 30000]
    with ThreadPoolExecutor(2) as pool:
        futures = [pool.submit(survey, k, kp[k]) for k in range(3)]
        together = [f.result() for f in futures]
    alone = [survey(k) for k in range(3)]
    for images, _ in views:
        ctx.synth_views_free(images)
    ctx.close()
    with open(out_path, "wb") as f:
        pickle.dump(dict(together=together, alone=alone), f)


def _run_child(tmp_path, handover, fail_middle=False):
    out = str(tmp_path / f"{handover}_{int(fail_middle)}.pkl")
    env = dict(os.environ, OCHIP_EXTRACT_HANDOVER=handover, OCHIP_EXTRACT_CHUNK="2",
               PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    env.pop("OCHIP_EXTRACT_GATE", None)
    env.pop("OCHIP_EXTRACT_STREAMS", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out, "1" if fail_middle else "0"], env=env,
                       capture_output=True, text=True, timeout=CHILD_SECONDS)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(out, "rb") as f:
        return pickle.load(f)


def test_slot_and_survey_handover_give_the_same_surveys(tmp_path):
    slot = _run_child(tmp_path, "slot")
    survey = _run_child(tmp_path, "survey")
    for k in range(3):
        feats, edges = slot["alone"][k]
        assert len(feats) == 9 and min(f[0] for f in feats) > 200 and len(edges) >= 16
        assert slot["together"][k] == slot["alone"][k]          # two threads == one after the other
        assert survey["together"][k] == survey["alone"][k]
        assert slot["together"][k] == survey["together"][k]     # per slot == per survey
    assert slot["alone"][0] != slot["alone"][1]                   # (the surveys are different views)


@pytest.mark.parametrize("handover", ["slot", "survey"])
def test_a_failing_survey_frees_its_slots(tmp_path, handover):
    got = _run_child(tmp_path, handover, fail_middle=True)
    kind, message = got["together"][1]
    assert kind == "error" and "max_kp" in message, message
    assert got["together"][0] == got["alone"][0]
    assert got["together"][2] == got["alone"][2]                # the survey after the failed one completes, unchanged
    assert len(got["alone"][1][0]) == 9                         # (and the same views extract with room for their keypoints)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2] == "1")
