"""bench.py's driver line: the last stdout line must be one JSON object under 8 KB
carrying the contract keys, `roofline` (numeric traffic) and `cpu_baseline`, built here from a
recorded full result of round 5 (profiles/r05/s5/bench.json, whose single 20-KB line the driver
could not parse)."""
import io
import json
import os
import contextlib

import pytest

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED = os.path.join(REPO, "profiles", "r05", "s5", "bench.json")

CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "config", "build", "roofline", "cpu_baseline")


def _recorded():
    if not os.path.exists(RECORDED):
        pytest.skip("recorded round-5 result not in this tree")
    with open(RECORDED) as f:
        return json.loads(f.read().strip().splitlines()[-1])


def test_compact_line_from_recorded_result(tmp_path):
    full = _recorded()
    assert len(json.dumps(full)) > bench.FINAL_LINE_MAX  # the case that failed in round 5
    details = str(tmp_path / "details.json")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.emit(full, details)
    lines = buf.getvalue().splitlines()
    assert len(lines) == 1
    line = lines[-1]
    assert len(line.encode()) <= bench.FINAL_LINE_MAX
    d = json.loads(line)
    for k in CONTRACT:
        assert k in d, k
    assert d["value"] == full["value"] and d["ms_per_step"] == full["ms_per_step"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r
    assert isinstance(r["traffic"], (int, float))
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], abs=1e-3)
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb
    assert cb["legs"]["dcn_4096"]["gpu_over_cpu"] >= 10  # the north star's DCN-4096 leg stays
    assert d["models"]["dcn"]["sps"] == full["models"]["dcn"]["samples_per_s"]
    assert "gather_frac" in d["models"]["deepfm"]
    # the side file holds every leg in full
    with open(details) as f:
        assert json.load(f) == full


def test_compact_line_falls_back_when_extras_grow(tmp_path):
    full = _recorded()
    full["models"] = {f"m{i}": {"samples_per_s": 1.0, "ms_per_step": 1.0, "roofline": {"frac": 0.5}}
                      for i in range(400)}
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.emit(full, str(tmp_path / "d.json"))
    line = buf.getvalue().splitlines()[-1]
    assert len(line.encode()) <= bench.FINAL_LINE_MAX
    d = json.loads(line)
    assert "models" not in d and d["roofline"]["frac"] == full["roofline"]["frac"]


LEG_SWITCHES = ("no_extras", "no_cpu", "no_sharded", "no_model_curve", "no_loader", "no_train")


def test_plain_run_times_the_headline_only():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs, a.details) == (7, 2, False, None, None)
    assert all(getattr(a, k) for k in LEG_SWITCHES)  # every leg beside the headline is off


def test_full_run_keeps_every_leg_and_its_switches():
    a = bench.parse(["--full"])
    assert a.full and not any(getattr(a, k) for k in LEG_SWITCHES)
    assert a.details == bench.DEFAULT_DETAILS
    b = bench.parse(["--full", "--no-cpu", "--details", "x.json", "--dump-outputs", "out"])
    assert b.no_cpu and not b.no_extras and b.details == "x.json" and b.dump_outputs == "out"


def test_dump_outputs_float32_arrays(tmp_path, monkeypatch):
    import numpy as np
    import torch
    prob = torch.rand(300, 1, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    d = str(tmp_path / "dump")
    info = bench.dump_outputs(d, ("prob", "l2_reg"), (prob, 0.25))
    assert info == {"dir": d, "arrays": {"prob": [300, 1], "l2_reg": []}}
    got = np.load(os.path.join(d, "prob.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, prob.numpy().astype(np.float32))
    l2 = np.load(os.path.join(d, "l2_reg.npy"))
    assert l2.dtype == np.float32 and l2.shape == () and l2 == np.float32(0.25)
    # past the size bound: the same sorted row sample on every run, within the bound
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 100 * 4)
    rows = []
    for _ in range(2):
        info = bench.dump_outputs(d, ("prob", "l2_reg"), (prob, 0.25))
        assert info["arrays"]["prob"] == [100, 1]
        rows.append(np.load(os.path.join(d, "prob.npy")))
    assert np.array_equal(rows[0], rows[1])
    full = prob.numpy().astype(np.float32)[:, 0]
    pos = np.searchsorted(np.sort(full), rows[0][:, 0])  # every sampled value is one of the rows
    assert np.array_equal(np.sort(full)[pos], rows[0][:, 0])
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 2 * 100 * 4 + 2 * 128


def test_counter_staleness_tags():
    bench._LIB_SRC = "abc"
    try:
        assert bench.counter_staleness({"src": "abc"}) == "current"
        assert bench.counter_staleness({"src": "def"}).startswith("stale")
        assert bench.counter_staleness({}) == "unknown"
    finally:
        bench._LIB_SRC = None
