"""DeepFM train step, dense against sparse table gradients, as one hipGraph per step.

Two shapes at B 4096: DeepFM configs[1]'s tables (30 fields x 1,000,000 rows x 32, the project's
large shape) and the WeChat tables (the vocabulary the training table of DESIGN.md uses).

  dense   the default path: zero-filled table-sized gradients, rk_embedding_backward, rankops.Adam
          over every parameter
  sparse  DeepFM(sparse_grad=True): sparse COO table gradients (one rk_pack_blocks launch),
          rankops.Adam on the dense parameters and rankops.SparseAdam on the tables

Per leg: the step time as the best of three windows of graph replays (host clock around a
synchronise, as the training table is timed), the windows themselves, and the peak memory
allocated during a step above what is held between steps, with the held bytes beside it.
Needs a GPU; prints one JSON line per shape and leg, and a summary line at the end."""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402,F401  (sets sys.path for rankops and tests/)
import torch  # noqa: E402

import helpers as H  # noqa: E402
import rankops  # noqa: E402

SHAPES = {
    "configs1": dict(dim=32, fields={f"field_{i:02d}": 1_000_000 for i in range(30)}),
    "wechat": dict(dim=8, fields={f: H.WECHAT_VOCAB[f] for f in rankops.deepfm.WECHAT_FIELDS}),
}


def leg(shape, sparse, batch, steps, warmup):
    cfg = SHAPES[shape]
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = rankops.DeepFM(None, embedding_dim=cfg["dim"], vocab_sizes=cfg["fields"], sparse_grad=sparse)
    model = model.cuda().train()
    inp = H.to_device(H.deepfm_inputs(batch, cfg["fields"], seed=77), "cuda")
    label = (torch.rand(batch, device="cuda") < 0.3).float()
    crit = torch.nn.BCELoss()
    if sparse:
        tables = [p for m in model.modules() if isinstance(m, torch.nn.Embedding) for p in m.parameters()]
        ids = {id(p) for p in tables}
        opts = [rankops.Adam([p for p in model.parameters() if id(p) not in ids], lr=1e-3, capturable=True),
                rankops.SparseAdam(tables, lr=1e-3, capturable=True)]
    else:
        opts = [rankops.Adam(model.parameters(), lr=1e-3, capturable=True)]

    def step():
        for o in opts:
            o.zero_grad(set_to_none=True)
        out = model(inp["category"])
        crit(out[0].squeeze(), label).backward()
        for o in opts:
            o.step()

    step()  # optimizer states and workspace
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    for o in opts:
        o.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()  # an eager step: what a step allocates on top of weights and optimizer state
    torch.cuda.synchronize()
    step_peak = torch.cuda.max_memory_allocated() - held
    for o in opts:
        o.zero_grad(set_to_none=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        step()
    for _ in range(warmup):
        g.replay()
    torch.cuda.synchronize()
    windows = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(steps):
            g.replay()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / steps)
    flags = rankops.error_flags()
    res = {"shape": shape, "leg": "sparse" if sparse else "dense", "batch": batch,
           "tables": len(cfg["fields"]) * 2, "rows_per_table": max(cfg["fields"].values()), "dim": cfg["dim"],
           "ms_per_step": round(1e3 * min(windows), 4), "windows_ms": [round(1e3 * w, 4) for w in windows],
           "held_between_steps_gb": round(held / 1e9, 3), "step_peak_above_held_gb": round(step_peak / 1e9, 4),
           "peak_allocated_gb": round((held + step_peak) / 1e9, 3), "error_flags": flags}
    del g, model, opts, inp
    gc.collect()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="configs1,wechat")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_train_time.py needs a ROCm GPU")
    summary = {}
    for shape in args.shapes.split(","):
        legs = {}
        for sparse in (False, True):
            r = leg(shape, sparse, args.batch, args.steps, args.warmup)
            print(json.dumps(r), flush=True)
            legs[r["leg"]] = r
        summary[shape] = {
            "dense_ms": legs["dense"]["ms_per_step"], "sparse_ms": legs["sparse"]["ms_per_step"],
            "dense_over_sparse": round(legs["dense"]["ms_per_step"] / legs["sparse"]["ms_per_step"], 2),
            "dense_peak_gb": legs["dense"]["peak_allocated_gb"], "sparse_peak_gb": legs["sparse"]["peak_allocated_gb"],
            "peak_saved_gb": round(legs["dense"]["peak_allocated_gb"] - legs["sparse"]["peak_allocated_gb"], 3)}
    print(json.dumps({"sparse_train_time": summary}), flush=True)


if __name__ == "__main__":
    main()
