"""DIEN at the reference shape (B 4096, T 50, H 16, nh 8, WeChat vocabulary), both cells: the time
of one rk_dien_interest launch, of the whole rankops.DIEN eval forward, and — the baseline, what a
user has without the kernel — of the same forward written as eager torch ops on the same GPU in
the same process (the per-step loop of tests/dien_ref.py in fp32).

Device times are HIP events around hipGraph replays (the host's launch cost excluded); the eager
loop is timed both as it runs (host clock around a synchronise: its ~1,300 launches are
host-bound) and captured in a graph.  The shader clock the device reports is printed beside them.
Needs a GPU; prints one JSON line at the end."""
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (sets sys.path for rankops and tests/)
import torch  # noqa: E402

import dien_ref  # noqa: E402
import helpers as H  # noqa: E402
import rankops  # noqa: E402
from rankops import _lib, ops  # noqa: E402

B, T = 4096, 50


def shader_clock():
    """The active sclk level the driver reports (read-only sysfs), or None."""
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            for line in open(path):
                if line.strip().endswith("*"):
                    return line.split(":", 1)[1].strip(" *\n")
        except OSError:
            pass
    return None


def graph_avg_ms(fn, iters=20):
    g, _ = bench.graph_of(fn)
    st = torch.cuda.current_stream()
    g.replay()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(st)
    for _ in range(iters):
        g.replay()
    end.record(st)
    end.synchronize()
    return start.elapsed_time(end) / iters


def host_avg_ms(fn, iters=5):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def main():
    assert torch.cuda.is_available(), "dien_time needs a ROCm GPU"
    rankops.load_library()
    result = {"B": B, "T": T, "H": 16, "nh": 8, "device": torch.cuda.get_device_name(0),
              "max_clock_khz": getattr(torch.cuda.get_device_properties(0), "clock_rate", None),
              "sclk_before": shader_clock()}
    inp = H.to_device(H.din_inputs(B, T, H.WECHAT_VOCAB, seed=1), "cuda")
    for cell in ("AGRU", "AUGRU"):
        torch.manual_seed(0)
        m = rankops.DIEN(None, custom_gru_type=cell, vocab_sizes=H.WECHAT_VOCAB)
        H.randomize_eval_stats(m, 1)
        m = m.cuda().eval()
        p = {k: v.detach() for k, v in m.state_dict().items()}
        args = (inp["dense"], inp["category"], inp["sequence"], inp["target"])

        def eager():
            return dien_ref.forward(p, *args, cell_type=cell, dtype=torch.float32)

        with torch.no_grad():
            prob, logit = m(*args)
            ref = eager()
            diff = (logit - ref[1]).abs().max().item()
            # the interest launch alone, bound as the module binds it
            pl = m._plan(*args)
            row = torch.empty(B, pl["width"], device="cuda")
            ops.concat_gather(pl["segs"], B, row)
            w = m.interest_weights()

            def launch():
                ops.dien_interest(_lib.fptr(row, pl["q_col"]), pl["width"], m.embeddings["feedid"].weight, pl["seq"],
                                  pl["seq_len"], T, 16, 8, ops.DIEN_CELLS[cell], w,
                                  _lib.fptr(row, pl["state_col"]), pl["width"], None, B, row.device)

            r = {"logit_max_abs_diff_vs_eager_fp32": diff,
                 "interest_launch_us": 1e3 * bench.graph_kernel_avg_ms(launch),
                 "forward_graph_us": 1e3 * graph_avg_ms(lambda: m(*args)),
                 "forward_eager_call_us": 1e3 * host_avg_ms(lambda: m(*args), iters=50),
                 "torch_loop_graph_us": 1e3 * graph_avg_ms(eager, iters=5),
                 "torch_loop_eager_us": 1e3 * host_avg_ms(eager)}
        r["torch_loop_graph_over_forward_graph"] = r["torch_loop_graph_us"] / r["forward_graph_us"]
        r["torch_loop_eager_over_forward_eager"] = r["torch_loop_eager_us"] / r["forward_eager_call_us"]
        result[cell] = r
        print(f"{cell}: " + ", ".join(f"{k} {v:.4g}" for k, v in r.items()), flush=True)
    result["sclk_after"] = shader_clock()
    assert rankops.error_flags() == 0
    print(json.dumps(result))


if __name__ == "__main__":
    main()
