"""ShardedDeepFM.train_step through a REAL torch.distributed process group (the pattern of
test_gpu_process_group.py): world 2 and 3, every rank a fresh child process on cuda:0 running
tests/dist_sharded_train_worker.py over gloo — at most four processes with the GPU open, pytest
included.  Each rank holds its parameters after each of two steps to the float64 restatement and
writes a JSON verdict; the ranks' dense-parameter checksums must agree (bit-identical replicas).
Every child runs under communicate(timeout=...); after a rank that failed or timed out the rest are
killed and nothing more is started."""
import json
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_ranks(world, tmp_path, timeout=180):
    port = _free_port()
    procs, outs = [], []
    for r in range(world):
        out = str(tmp_path / f"rank{r}.json")
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), RK_OUT=out)
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "dist_sharded_train_worker.py")],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
        outs.append(out)
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=timeout)[0].decode(errors="replace")[-2000:])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    res = []
    for r, out in enumerate(outs):
        if not os.path.exists(out):
            res.append({"rank": r, "ok": False, "error": "no result", "log": logs[r] if r < len(logs) else ""})
        else:
            with open(out) as f:
                res.append(json.load(f))
    return res, [p.returncode for p in procs]


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_sharded_train_step_real_process_group(world, tmp_path):
    res, rcs = _run_ranks(world, tmp_path)
    bad = [r for r in res if not r.get("ok")]
    assert not bad, json.dumps(bad, indent=1)[:6000]
    assert rcs == [0] * world
    assert len({r["dense_checksum"] for r in res}) == 1, [r["dense_checksum"] for r in res]
    print("all_reduce path:", {r["all_reduce"] for r in res})
