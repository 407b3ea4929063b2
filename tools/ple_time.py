"""Times of the PLE eval forward at B 4096 and 32,768 with the wechat tables, for the default configuration
(L = 2; 3 tasks, 2 specific + 2 shared experts 256-128 per level, towers 64) and for L = 3, three ways, in one
process:

  (a) kernel    rk_ple_forward, the one launch rankops.PLE runs
  (b) torch     the float32 torch-ROCm formulation of the same module (embedding lookups, cat, every level's
                nn.Sequential experts, softmax gates and einsum mixes, the towers, sigmoid)
  (c) composed  the same forward from the launches the engine had before this kernel: rk_concat_gather, per
                level one rk_mlp_forward per expert on its own input, torch addmm + softmax for the gates and
                einsum for the mixes, then one rk_mlp_forward per tower (with its head).  This composition
                lives here only.

The method is tools/mmoe_time.py's: every leg is captured in a hipGraph once and timed as replays between
device events; the legs alternate and the median over the rounds is reported with the fastest and slowest
round.  The three are compared with each other before anything is timed.  From the shapes the tool computes
the forward's flops per sample and reports the kernel's rate as a share of the 157.3 TF FP32 matrix peak of
the MI355X (the MFMA FP32 peak, not a measured ceiling).  `--batches 2048,8192` measures other batch sizes;
`--legs kernel` times leg (a) alone.  Needs a GPU; prints one JSON line at the end.

`--train` times one training step instead (forward + backward of BCE-with-logits over the K label columns,
gradients set to None first, optimizer excluded) at the same four points, two legs by the same method
(tools/mmoe_time.py --train's):

  (a) engine    rankops.PLE(trainable=True) in train mode: rk_ple_forward_train and ops.ple_backward
  (b) torch     float32 torch autograd of the same module (torch_forward in train mode: nn.Dropout live)

with the same dropout rate (a whole step captured with dien_time.grad_graph_of), and prints the launches of
one eager step of (a), counted on the host (tests/launch_count.py's launches_of) — their number depends on L,
the depths and ceil((K ms + mc) / 16) only."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (sets sys.path for rankops and tests/)
import torch  # noqa: E402

import helpers as H  # noqa: E402
import rankops  # noqa: E402
from rankops import common, ops  # noqa: E402

from dien_time import grad_graph_of, shader_clock  # noqa: E402
from launch_count import launches_of  # noqa: E402  (tests/launch_count.py)
from mmoe_time import FP32_MATRIX_PEAK_TF, ROUNDS, replay_us  # noqa: E402


def flops_per_sample(model):
    def stack(width, units):
        total = 0
        for n in units:
            total += 2 * width * n
            width = n
        return total, width
    K, ms, mc = len(model.task_names), model.num_specific_experts, model.num_shared_experts
    NE, H_ = K * ms + mc, model.expert_hidden_units[-1]
    total = 0
    for j in range(model.num_levels):
        width = model.input_dim if j == 0 else H_
        last = j == model.num_levels - 1
        gate_cols = K * (ms + mc) + (0 if last else NE)
        total += NE * stack(width, model.expert_hidden_units)[0] + 2 * width * gate_cols + 2 * gate_cols * H_
    tw, end = stack(H_, model.tower_hidden_units)
    return total + K * (tw + 2 * end)


def torch_forward(model, dense, cat):
    x = torch.cat([dense] + [emb(cat[n]) for n, emb in model.embeddings.items()], dim=1)
    K = len(model.task_names)
    xk, xs = [x] * K, x
    for level in model.levels:
        fk = [[e(xk[k]) for e in level.specific_experts[k]] for k in range(K)]
        fs = [e(xs) for e in level.shared_experts]
        new = [torch.einsum("bc,bch->bh", torch.softmax(level.gates[k](xk[k]), dim=1), torch.stack(fk[k] + fs, dim=1))
               for k in range(K)]
        if hasattr(level, "shared_gate"):
            xs = torch.einsum("bc,bch->bh", torch.softmax(level.shared_gate(xs), dim=1),
                              torch.stack([f for task in fk for f in task] + fs, dim=1))
        xk = new
    logits = torch.cat([out(tower(xk[k])) for k, (tower, out) in enumerate(zip(model.towers, model.tower_outputs))],
                       dim=1)
    return torch.sigmoid(logits), logits


def composed_forward(model, dense, cat):
    """Leg (c): its buffers and marshalled layers, and the function that runs it."""
    B, dev = dense.shape[0], dense.device
    K, ms, mc = len(model.task_names), model.num_specific_experts, model.num_shared_experts
    NE, Hw = K * ms + mc, model.expert_hidden_units[-1]
    segs = [ops.dense_segment(dense, model.num_dense_features, 0)]
    col = model.num_dense_features
    for n, emb in model.embeddings.items():
        segs.append(ops.table_segment(emb.weight, cat[n], col))
        col += emb.embedding_dim
    x = torch.empty(B, model.input_dim, device=dev)
    f = torch.empty(B, NE, Hw, device=dev)
    logits, probs = torch.empty(K, B, device=dev), torch.empty(K, B, device=dev)

    def layers(seq):
        return [ops.make_mlp_layer(l.weight, common.PACKED(l.weight), bias=l.bias, act="relu")
                for l in seq if isinstance(l, torch.nn.Linear)]
    experts = [[layers(seq) for seq in level.stacks()] for level in model.levels]
    towers = [layers(seq) for seq in model.towers]
    heads = [ops.make_epilogue(head_w=o.weight, head_b=o.bias, head_logit=logits[k], head_prob=probs[k])
             for k, o in enumerate(model.tower_outputs)]
    owner = [s // ms if s < K * ms else K for s in range(NE)]
    columns = [torch.tensor(list(range(k * ms, (k + 1) * ms)) + list(range(K * ms, NE)), device=dev) for k in range(K)]

    def run():
        ops.concat_gather(segs, B, x)
        inputs = [x] * (K + 1)
        for j, level in enumerate(model.levels):
            for s in range(NE):
                ops.mlp_forward(inputs[owner[s]], experts[j][s], None, f[:, s])
            new = [torch.einsum("bc,bch->bh", torch.softmax(torch.addmm(g.bias, inputs[k], g.weight.t()), dim=1),
                                f.index_select(1, columns[k])) for k, g in enumerate(level.gates)]
            if hasattr(level, "shared_gate"):
                g = level.shared_gate
                new.append(torch.einsum("bc,bch->bh", torch.softmax(torch.addmm(g.bias, inputs[K], g.weight.t()), dim=1), f))
            inputs = new
        for k in range(K):
            ops.mlp_forward(inputs[k], towers[k], heads[k])
        return probs, logits
    run.keep = (segs, experts, towers, heads)
    return run


def measure(L, B):
    torch.manual_seed(42)
    model = rankops.PLE(None, num_levels=L, vocab_sizes=H.WECHAT_VOCAB).cuda().eval()
    inp = H.to_device(H.dcn_inputs(B, H.WECHAT_VOCAB, 1000), "cuda")
    dense, cat = inp["dense"], inp["category"]
    dev = dense.device
    names, idx = model._indices(cat)
    built = model._build(dense, names, idx)
    out = model._outputs(B, dev)

    def kernel():
        model._run(built, out, ops._lib.raw_stream(dev))
        return out
    composed = composed_forward(model, dense, cat)
    fns = {"kernel": kernel, "torch": lambda: torch_forward(model, dense, cat), "composed": composed}
    if "--legs" in sys.argv[1:]:
        fns = {k: fns[k] for k in sys.argv[sys.argv.index("--legs") + 1].split(",")}
    with torch.no_grad():
        prob_a, logit_a = [t.clone() for t in kernel()]
        prob_b, logit_b = torch_forward(model, dense, cat)
        prob_c, logit_c = [t.t().clone() for t in composed()]
    torch.cuda.synchronize()
    err_b = float(((logit_a - logit_b).abs() / (1 + logit_b.abs())).max())
    err_c = float(((logit_a - logit_c).abs() / (1 + logit_c.abs())).max())
    assert err_b <= 1e-4 and err_c <= 1e-4, f"legs differ: kernel vs torch {err_b}, kernel vs composed {err_c}"
    assert float((prob_a - prob_b).abs().max()) <= 1e-4
    with torch.no_grad():
        graphs = {k: bench.graph_of(fn)[0] for k, fn in fns.items()}
    times = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            times[k].append(replay_us(g))
    r = {}
    for k, t in times.items():
        r[f"{k}_us"] = {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
    med = {k: statistics.median(t) for k, t in times.items()}
    flops = flops_per_sample(model)
    r["flops_per_sample"] = flops
    r["kernel_tflops"] = round(flops * B / med["kernel"] / 1e6, 2)
    r["share_of_fp32_matrix_peak"] = round(flops * B / med["kernel"] / 1e6 / FP32_MATRIX_PEAK_TF, 4)
    if "torch" in med:
        r["torch_over_kernel"] = round(med["torch"] / med["kernel"], 2)
    if "composed" in med:
        r["composed_over_kernel"] = round(med["composed"] / med["kernel"], 2)
    r["kernel_vs_torch_max_rel_err"], r["kernel_vs_composed_max_rel_err"] = err_b, err_c
    del graphs, model
    torch.cuda.empty_cache()
    return r


def measure_train(L, B):
    torch.manual_seed(42)
    engine = rankops.PLE(None, num_levels=L, vocab_sizes=H.WECHAT_VOCAB, trainable=True).cuda().train()
    torch.manual_seed(42)
    plain = rankops.PLE(None, num_levels=L, vocab_sizes=H.WECHAT_VOCAB).cuda().train()
    inp = H.to_device(H.dcn_inputs(B, H.WECHAT_VOCAB, 1000), "cuda")
    dense, cat = inp["dense"], inp["category"]
    K = len(engine.task_names)
    labels = (torch.rand(B, K, generator=torch.Generator().manual_seed(3)) < 0.3).float().cuda()
    crit = torch.nn.BCEWithLogitsLoss()

    def step_of(model, forward):
        def step():
            with torch.enable_grad():
                for prm in model.parameters():
                    prm.grad = None
                crit(forward()[1], labels).backward()
        return step
    fns = {"engine": step_of(engine, lambda: engine(dense, cat)),
           "torch": step_of(plain, lambda: torch_forward(plain, dense, cat))}
    graphs = {k: grad_graph_of(fn) for k, fn in fns.items()}
    times = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            times[k].append(replay_us(g))
    r = {}
    for k, t in times.items():
        r[f"{k}_us"] = {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
    med = {k: statistics.median(t) for k, t in times.items()}
    r["torch_over_engine"] = round(med["torch"] / med["engine"], 2)
    r["torch_over_engine_range"] = [round(min(times["torch"]) / max(times["engine"]), 2),
                                    round(max(times["torch"]) / min(times["engine"]), 2)]
    del graphs
    names = launches_of(fns["engine"])  # after the timing: nothing of the count runs before a capture
    r["engine_launches"] = len(names)
    r["engine_launch_list"] = names
    del engine, plain
    torch.cuda.empty_cache()
    return r


def main():
    assert torch.cuda.is_available(), "ple_time needs a ROCm GPU"
    rankops.load_library()
    result = {"device": torch.cuda.get_device_name(0), "fp32_matrix_peak_tf": FP32_MATRIX_PEAK_TF,
              "sclk_before": shader_clock()}
    batches = (4096, 32768)
    if "--batches" in sys.argv[1:]:
        batches = tuple(int(b) for b in sys.argv[sys.argv.index("--batches") + 1].split(","))
    for L in (2, 3):
        for B in batches:
            r = measure_train(L, B) if "--train" in sys.argv[1:] else measure(L, B)
            result[f"L{L}_B{B}"] = r
            print(f"L {L} B {B}: " + ", ".join(f"{k} {v}" for k, v in r.items()), flush=True)
    result["sclk_after"] = shader_clock()
    assert rankops.error_flags() == 0
    print(json.dumps(result))


if __name__ == "__main__":
    main()
