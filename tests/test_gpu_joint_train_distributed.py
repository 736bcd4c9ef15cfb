"""The data-parallel JOINT step executed on the GPU box: two ranks over gloo on the one GPU, and one rank on RCCL
(tests/dist_joint_train_check.py; the ranks are fresh child processes started by torch.distributed.run)."""
import os
import re
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join("tests", "dist_joint_train_check.py")


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(script_args, nproc=2, timeout=600):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port())] + script_args
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    return subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("L", [3, 4])
def test_two_rank_joint_step_averages_the_whole_bucket(L):
    """L = 3: no side stream, the mask segment's early all-reduce and one more; L = 4: three collectives, the message-passing
    bucket's ordered behind the library's side stream."""
    r = run_ranks([CHILD, "average", str(L)])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert len(re.findall(r"RANK \d joint err", r.stdout)) == 2, r.stdout[-2000:]


def test_invalid_graph_on_one_rank_stops_the_joint_step_everywhere():
    r = run_ranks([CHILD, "badgraph", "3"])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "RANK 1 joint badgraph raised 1 unchanged 1 applied 0" in r.stdout and \
        "RANK 0 joint badgraph raised 0 unchanged 1 applied 0" in r.stdout, r.stdout[-2000:]


def test_one_rank_rccl_group_runs_the_joint_collectives():
    r = run_ranks([CHILD, "nccl1", "4"], nproc=1)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "NCCL1 joint ok 1 mask_collectives 2" in r.stdout, r.stdout[-2000:]
