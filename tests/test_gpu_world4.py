"""Four ranks on the one GPU of the test box (gloo transport, the ranks share cuda:0): one survey from pixels over the
ranks, its relaxes sharded, the clustered stage's groups dealt over the ranks - two groups per rank
(tests/sharded_world4_worker.py).  Two RCCL ranks have never run (1-GPU boxes); this keeps everything around the transport -
block arithmetic, exchanges, groups dealt over fewer ranks than groups - exercised beyond N = 2.  Four ranks and this
process stay within the six processes that may hold a shared GPU open at once (`bench.py --gpus N --full` runs a
strong-mode child beside every rank, so its launcher form is tested at N = 2, tests/test_gpu_survey_sharded.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_four_ranks_survey_relaxes_and_groups():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=4", "--master-addr", "127.0.0.1",
           "--master-port", "29571", os.path.join(ROOT, "tests", "sharded_world4_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2", OCHIP_HOST_THREADS="2")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1800, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "WORLD4 OK" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]

