"""Digests of six small relax solves that between them take every kernel and host path using the shared LM step rules
(csrc/relax_lm_rules.hpp): SHA-256 of the final state (orientations, heights / surface, lens parameters, points) and the
figures of the solves (solves, LM iterations, and termination / successful / unsuccessful steps where the interface gives
them; the initial and final costs to the bit elsewhere).  Two builds that print the same lines compute the same relax.
usage: relax_rules_digest.py [--root DIR] [--out FILE]     (DIR: a checkout with its libraries built; default: this one)

  plane        the plane relax of a 3 x 8 synthetic grid (pair-record engine, speculative steps, tail candidate)
  mesh_stage   the GROUND_MESH relax stage of the same grid (general engine)
  intrinsics   ORIENTATION + GROUND_MESH + FOCAL_LENGTH on the 4 x 5 track grid of tests/test_gpu_relax_intrinsics.py, two
               rounds (general engine, bounds: the projected line search)
  points       the smallest scene of tests/relaxp_eval_fixtures.py solved by the points engine (Schur elimination, bounds)
  chain        the 3 x 8 / batch 8 bootstrap schedule through the resident chain (small-system and tile routes)
  host_loop    the same schedule through the host loop (OCHIP_TEST_HOOKS=host_bootstrap)"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
args = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the library under test from --root; the fixtures (data only) from this checkout
sys.path[:0] = [os.path.abspath(args.root), os.path.join(HERE, "tests")]
from opencalibration_amd import capi, host, pipeline, synth  # noqa: E402

import relaxp_eval_fixtures as PF  # noqa: E402
from relax_fixtures import axis_angle, camera_grid_tracks, features_of_edges, qmul  # noqa: E402


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.float64).tobytes())
    return h.hexdigest()


def bits(x):
    return np.float64(x).tobytes().hex()


def figures(r):
    return [int(r["solves"]), int(r["iterations_total"]), int(r["last_iterations"]), int(r["residual_blocks"]),
            bits(r["initial_cost"]), bits(r["final_cost"])]


def surface_arrays(s):
    a = s.arrays()
    return a["vertices"], a["cloud"]


ctx = capi.Context(0)
out = {}

grid = synth.make_grid(3, 8, feats=512, seed=11)
g = host.Graph.from_synthetic(grid)
start = pipeline.perturbed_orientations(grid, 0.1, 99)
g.set_orientations(start)
g.link(ctx)
plane = g.relax(ctx, start, host.relax_options("ORIENTATION", "GROUND_PLANE"))
out["plane"] = dict(state=sha(plane["orientation"], *surface_arrays(plane["surface"])), figures=figures(plane))

g.set_orientations(plane["orientation"])
seed_mesh = host.rebuild_mesh(grid.position, plane["surface"], minimal=True)
st = g.relax_stage(ctx, host.relax_options("ORIENTATION", "GROUND_MESH"), 0.1, previous=seed_mesh)
out["mesh_stage"] = dict(state=sha(g.orientations(), *surface_arrays(st["surface"])), figures=figures(st) + [int(st["groups"])])
g.close()

ori, pos, edges, model = camera_grid_tracks(4, 5, pts_per_side=18)
rng = np.random.default_rng(2)
for e in edges:
    e["px"] = e["px"] + rng.normal(0, 0.2, e["px"].shape)
n = len(pos)
q = np.array([qmul(ori[i], axis_angle(rng.normal(size=3) / 2, 0.02)) for i in range(n)])
off = model.copy()
off[0] *= 1.03
gx = np.linspace(-4, 14, 8)
cloud = np.array([[x, y, 1e-3 * x + 1e-2 * y] for x in gx for y in gx])
feats, plan = features_of_edges(n, edges)
pk = host.pack_edges(edges)
pk["feat"] = np.concatenate([np.stack([f1, f2], 1) for f1, f2 in plan]).astype(np.uint64)
prev = host.Surface()
prev.set(np.zeros((0, 3)), np.zeros((0, 5), np.uint64), cloud)
hm, figs = np.array(off, float), []
for r in range(2):
    h = host.relax(ctx, pos, ori, off, feats, np.arange(n), q, pk,
                   host.relax_options("ORIENTATION", "GROUND_MESH", "FOCAL_LENGTH"), 0.1, previous=prev, cam_model=hm)
    q, hm, prev = h["orientation"], h["cam_model"], h["surface"]
    figs += figures(h)
out["intrinsics"] = dict(state=sha(q, hm, *surface_arrays(prev)), figures=figs)

scene = PF.functor(0)
p = ctx.relaxp_evaluate(scene, iterations=100, radius=1e4)
s = p["summary"]
out["points"] = dict(state=sha(p["cam_q"], p["point_xyz"], p["model"]),
                     figures=[1, int(s["iterations"]), int(s["termination"]), int(s["successful_steps"]), int(s["unsuccessful_steps"]),
                              bits(s["initial_cost"]), bits(s["final_cost"])])


def schedule(hook):
    if hook:
        os.environ["OCHIP_TEST_HOOKS"] = hook
    else:
        os.environ.pop("OCHIP_TEST_HOOKS", None)
    opts = host.relax_options("ORIENTATION", "GROUND_PLANE")
    g = host.Graph()
    m = g.add_model(grid.model)
    states, figs = [], []
    for lo in range(0, grid.n_images, 8):
        idx = list(range(lo, min(lo + 8, grid.n_images)))
        for i in idx:
            loc, st_, de, _ = grid.image(i)
            g.add_image(loc, st_, de, grid.num_sparse[i], m, grid.position[i])
        o = g.orientations().copy()
        o[lo:] = np.nan
        g.set_orientations(o)
        g.link(ctx, node_ids=[g.node_ids[i] for i in idx])
        r = g.relax_stage(ctx, opts, node_ids=[g.node_ids[i] for i in idx], disable_parallelism=True)
        states.append(g.orientations().copy())
        figs.append(figures(r))
    g.close()
    os.environ.pop("OCHIP_TEST_HOOKS", None)
    return dict(state=sha(*states), figures=figs)


out["chain"] = schedule(None)
out["host_loop"] = schedule("host_bootstrap")
ctx.close()

for k, v in out.items():
    print(k, v["state"], json.dumps(v["figures"]))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
