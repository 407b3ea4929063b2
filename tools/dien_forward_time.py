"""What the one-launch DIEN eval forward (rk_dien_forward) gains over the three launches it replaces,
at T 50, H 16, nh 8 with the WeChat vocabulary, both cells, B 4096 and 32,768, in one process:

  (a) the three launches (rankops.common.FUSED_DIEN = False): a hipGraph of 20 forwards replayed, and
      the forward as called;
  (b) the one launch (FUSED_DIEN = True), the same two ways;
  (c) DIEN.prepare's run(), as called.

Graph times are HIP events around replays (the host's launch cost excluded), per forward; "as called"
is the host clock around a synchronise, per forward.  Every leg is measured in two alternating rounds
(a, b, c, a, b, c) and both figures are printed: their spread is the noise the comparison has to beat.
The outputs of (b) and (c) are compared with (a)'s before anything is timed, and the shader clock the
driver reports is read before and after.  `--batches 2048,8192` measures other batch sizes.  Needs a
GPU; prints one JSON line at the end."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (sets sys.path for rankops and tests/)
import torch  # noqa: E402

import helpers as H  # noqa: E402
import rankops  # noqa: E402
from rankops import common  # noqa: E402

from dien_time import host_avg_ms, shader_clock  # noqa: E402

T, PER_GRAPH, ROUNDS = 50, 20, 2


def graph_us(fn, iters=10):
    """Device time of one call of fn: PER_GRAPH calls in one hipGraph, replayed."""
    g, _ = bench.graph_of(lambda: [fn() for _ in range(PER_GRAPH)])
    st = torch.cuda.current_stream()
    g.replay()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(st)
    for _ in range(iters):
        g.replay()
    end.record(st)
    end.synchronize()
    return 1e3 * start.elapsed_time(end) / (iters * PER_GRAPH)


def measure(cell, B):
    torch.manual_seed(0)
    m = rankops.DIEN(None, custom_gru_type=cell, vocab_sizes=H.WECHAT_VOCAB)
    H.randomize_eval_stats(m, 1)
    m = m.cuda().eval()
    inp = H.to_device(H.din_inputs(B, T, H.WECHAT_VOCAB, seed=1), "cuda")
    args = (inp["dense"], inp["category"], inp["sequence"], inp["target"])

    def forward(fused):
        def fn():
            common.FUSED_DIEN = fused
            with torch.no_grad():
                return m(*args)
        return fn

    three, fused = forward(False), forward(True)
    run = m.prepare(*args)
    want = three()
    for name, got in (("fused", fused()), ("prepared", run())):
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{name} differs from the three launches"
    assert not m.__dict__.get("_unfusable")
    legs = {"three_graph_us": lambda: graph_us(three), "fused_graph_us": lambda: graph_us(fused),
            "three_called_us": lambda: 1e3 * host_avg_ms(three, iters=50),
            "fused_called_us": lambda: 1e3 * host_avg_ms(fused, iters=50),
            "prepared_called_us": lambda: 1e3 * host_avg_ms(run, iters=50)}
    r = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, leg in legs.items():
            r[k].append(round(leg(), 2))
    spread = max(abs(v[0] - v[1]) for k, v in r.items() if k.endswith("graph_us"))
    r["graph_round_spread_us"] = round(spread, 2)
    r["fused_minus_three_graph_us"] = round(sum(r["fused_graph_us"]) / ROUNDS - sum(r["three_graph_us"]) / ROUNDS, 2)
    return r


def main():
    assert torch.cuda.is_available(), "dien_forward_time needs a ROCm GPU"
    rankops.load_library()
    default = common.FUSED_DIEN, common.FUSED_DIEN_WG_PER_CU
    common.FUSED_DIEN_WG_PER_CU = None  # (b) is the one launch at every batch measured
    result = {"T": T, "H": 16, "nh": 8, "device": torch.cuda.get_device_name(0), "sclk_before": shader_clock()}
    batches = (4096, 32768)
    if "--batches" in sys.argv[1:]:  # e.g. --batches 2048,8192: where the one launch stops winning
        batches = tuple(int(b) for b in sys.argv[sys.argv.index("--batches") + 1].split(","))
    for B in batches:
        for cell in ("AGRU", "AUGRU"):
            r = measure(cell, B)
            result[f"{cell}_B{B}"] = r
            print(f"{cell} B {B}: " + ", ".join(f"{k} {v}" for k, v in r.items()), flush=True)
    common.FUSED_DIEN, common.FUSED_DIEN_WG_PER_CU = default
    result["sclk_after"] = shader_clock()
    assert rankops.error_flags() == 0
    print(json.dumps(result))


if __name__ == "__main__":
    main()
