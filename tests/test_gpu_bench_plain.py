"""GPU: a plain bench.py run (no --full) times the DIN headline only, and --dump-outputs writes
what its last timed step computed: the (prob, logit, l2_reg) that an eager forward of the same
seeded model and inputs returns (the prepared launch equals the eager forward bit for bit,
test_gpu_din_plan.py)."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

import bench
import helpers as H

FULL_ONLY = ("roofline", "models", "loader", "train", "eval_metrics", "sharded_deepfm", "cpu_baseline", "details")


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # a plain run writes nothing but the dump
    tf32 = torch.backends.cuda.matmul.allow_tf32
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            bench.main(["--gpus", "1", "--steps", "6", "--warmup", "2", "--dump-outputs", "dump"])
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32
    lines = buf.getvalue().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "samples/s" and d["dtype"] == "f32"
    assert d["higher_is_better"] is True and d["steps"] == 6 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(4096 / (d["ms_per_step"] * 1e-3), rel=1e-2)  # both rounded from one window
    for k in FULL_ONLY:
        assert k not in d, k
    assert d["config"]["graph_replay_ms_per_step"] is None
    assert sorted(os.listdir(tmp_path)) == ["dump"]
    assert sorted(os.listdir(tmp_path / "dump")) == ["l2_reg.npy", "logit.npy", "prob.npy"]
    got = {n: np.load(tmp_path / "dump" / f"{n}.npy") for n in bench.OUTPUT_NAMES}
    assert d["outputs"]["arrays"] == {"prob": [4096, 1], "logit": [4096, 1], "l2_reg": []}

    # the same workload, built again from its seeds, through the eager forward
    model, inp, fn, cfg, name = bench.workload("din", 4096, 0)
    with torch.no_grad():
        want = H.as_tuple(fn())
    torch.cuda.synchronize()
    for n, w in zip(bench.OUTPUT_NAMES, want):
        assert got[n].dtype == np.float32
        assert np.array_equal(got[n], w.cpu().numpy()), n
    assert np.isfinite(got["prob"]).all() and got["prob"].std() > 0
