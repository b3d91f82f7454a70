"""Runs among the first -m gpu tests (file name order), before this pytest process has touched the GPU: fresh child
processes -- one per rank, all on the box's single GPU -- render the rt_aov_film planes of their tiles and gather them
with FilmGather.gather_planes over gloo (tools/aov_mp_check.py); rank 0 compares them with the one-rank planes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_gather_the_one_rank_planes():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = ["timeout", "-k", "10", "540", sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29531",
           os.path.join(ROOT, "tools", "aov_mp_check.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["ranks"] == 2 and rec["bit_identical"] and len(rec["planes"]) == 6
