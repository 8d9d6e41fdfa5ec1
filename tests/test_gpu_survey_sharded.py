"""ONE survey over 2 ranks from pixels (BASELINE config C4): extraction by image block, links by
owning rank, two all-gathers, sharded relax - everything equal to the single-process run bit for bit; and bench.py's
launcher + strong mode (`bench.py --gpus 2 --scaling strong`) end to end on the 200-image grid."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_worker(grid, port):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "sharded_survey_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="8", SHARD_TEST_GRID=grid)
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "SHARDED_SURVEY OK" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def test_two_ranks_one_survey_from_pixels():
    _run_worker("4x6", 29551)


def test_two_ranks_one_survey_uneven_blocks():
    _run_worker("3x5", 29553)     # 15 images: blocks of 8 and 7, a block border inside a strip


@pytest.mark.parametrize("relax", ["pipelined", "sharded"])
def test_bench_launches_its_ranks_strong(relax):
    """`bench.py --gpus 2` with no launcher around it starts two ranks (gloo, sharing the GPU) and prints one line."""
    env = dict(os.environ, OCHIP_BENCH_BACKEND="gloo", OCHIP_HOST_THREADS="8")
    env.pop("WORLD_SIZE", None), env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--scaling", "strong", "--relax", relax, "--config", "C2",
           "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["value"] > 0
    ss = line["strong_scaling"]
    assert len(ss["seconds_per_step_per_rank"]) == 2 and ss["bytes_gathered_per_step"] > 0
    assert line["relax"]["median_orientation_error_rad_vs_truth"] < 1e-3
    if relax == "sharded":  # the general engine (mesh flavour) ran behind the same exchange, once, in the warm-up step
        ge = ss["general_engine_sharded"]
        assert "error" not in ge, ge
        assert ge["ranks"] == 2 and ge["lm_iterations"] > 0 and ge["equals_the_unsharded_solve_bit_for_bit"]


def test_bench_weak_line_carries_the_strong_section():
    """`bench.py --gpus 2 --full` (the scaling run's command): one weak line, and beside it the strong mode run by a child
    process per rank (so that nothing it does can take the headline with it)."""
    env = dict(os.environ, OCHIP_BENCH_BACKEND="gloo", OCHIP_HOST_THREADS="8")
    env.pop("WORLD_SIZE", None), env.pop("RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "C2", "--steps", "2", "--warmup", "1", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0
    ss = line["strong_scaling"]
    assert "error" not in ss, ss
    assert ss["images_per_s"] > 0 and len(ss["seconds_per_step_per_rank"]) == 2
    # both curves by name at the top level, and the collective pre-flight ran
    assert line["images_per_s_weak_one_survey_per_gpu"] == line["value"]
    assert line["images_per_s_strong_one_survey_over_all_gpus"] == ss["images_per_s"]
    assert line["collective_preflight_s"] is not None and line["rccl_ranks"] == 0     # (gloo here)


def test_one_rank_strong_equals_the_default_line():
    """At N = 1 "one survey over all GPUs" and "a survey per GPU" are the same job: the strong mode's rate must agree with
    the default line's within run-to-run noise (both modes run the C2 grid here, relax pipelined over surveys)."""
    env = dict(os.environ, OCHIP_HOST_THREADS="8")
    env.pop("WORLD_SIZE", None), env.pop("RANK", None)
    def measure():
        rates = {}
        for mode in ("weak", "strong"):
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--scaling", mode, "--config", "C2", "--steps", "6", "--warmup", "2",
                   "--no-cpu-baseline"]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
            assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
            line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
            assert line["n_gpus"] == 1 and line["scaling"] == mode
            rates[mode] = line["value"]
        return rates

    # (six 50 ms steps of a 200-image grid under the box's CPU quota: one of the two runs is moved by more than the tolerance
    # now and then, in either direction.  What must hold is that neither mode is systematically slower: the best rate of
    # each mode over up to four measurements of the pair, which a slow run cannot lower)
    best = {"weak": 0.0, "strong": 0.0}
    seen = []
    for _ in range(4):
        rates = measure()
        seen.append(rates)
        for mode in best:
            best[mode] = max(best[mode], rates[mode])
        if abs(best["strong"] / best["weak"] - 1.0) < 0.15:
            break
    assert abs(best["strong"] / best["weak"] - 1.0) < 0.15, seen
