"""Times of the ESMM eval forward at B 4096 and 32,768 with the wechat tables, at the default shape
(K = 2, towers 256-128-64) and at K = 4 with towers 512-256-128, three ways, in one process:

  (a) kernel    rk_esmm_forward, the one launch rankops.ESMM runs
  (b) torch     the float32 torch-ROCm formulation of the same module (embedding lookups, cat, the towers'
                nn.Sequential, sigmoid, cumprod)
  (c) composed  the same forward from the launches the engine had before this kernel: one
                rk_mlp_forward_gather per tower (each gathers the row again and ends in its head), then
                torch's sigmoid and cumprod.  This composition lives here only.

Every leg is captured in a hipGraph once (after warm calls on a side stream) and timed as replays
between device events; the legs alternate — a, b, c, a, b, c, … — and the median over the rounds is
reported with the fastest and slowest round, whose spread is the noise a ratio has to beat.  The three
are compared with each other before anything is timed.

From the shapes the tool computes the forward's flops per sample (towers and heads) and reports the
kernel's rate as a share of the 157.3 TF FP32 matrix peak of the MI355X (the MFMA FP32 peak, not a
measured ceiling).  `--batches 2048,8192` measures other batch sizes.  Needs a GPU; prints one JSON line at
the end.

`--train` times one whole training step instead (gradients set to None, forward, the entire-space loss,
backward, Adam) at the same four points, two legs by the same method:

  (a) engine    rankops.ESMM(trainable=True) in train mode, rankops.esmm_loss, rankops.Adam
  (b) torch     float32 torch autograd of the same module (nn.Dropout live) with the log-domain loss
                written in torch ops (-(y S + (1 - y) log1p(-exp(S))), S = cumsum(logsigmoid(z)) clamped
                below 0) and torch.optim.Adam(capturable=True)

and prints the launches of one eager forward + loss + backward of (a), counted on the host
(tests/launch_count.py's launches_of), whose number must not depend on K."""
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

SHAPES = {"default": {}, "K4_512": dict(tower_hidden_units=(512, 256, 128),
                                        task_names=("click", "cart", "order", "purchase"))}


def flops_per_sample(model):
    total, width = 0, model.input_dim
    for n in model.tower_hidden_units:
        total += 2 * width * n
        width = n
    return len(model.task_names) * (total + 2 * width)


def torch_forward(model, dense, cat):
    x = torch.cat([dense] + [emb(cat[n]) for n, emb in model.embeddings.items()], dim=1)
    logits = torch.cat([out(tower(x)) for tower, out in zip(model.towers, model.tower_outputs)], dim=1)
    return torch.cumprod(torch.sigmoid(logits), dim=1), logits


def composed_forward(model, dense, cat):
    """Leg (c): its buffers and marshalled layers, and the function that runs it."""
    B, dev = dense.shape[0], dense.device
    K = len(model.task_names)
    names, idx = model._indices(cat)
    segs = model._segments(dense, names, idx)
    logits = torch.empty(K, B, device=dev)
    lib = ops._lib.load()
    calls, keep = [], []
    for k, (seq, o) in enumerate(zip(model.towers, model.tower_outputs)):
        layers = [ops.make_mlp_layer(l.weight, common.PACKED(l.weight), bias=l.bias, act="relu")
                  for l in seq if isinstance(l, torch.nn.Linear)]
        head = ops.make_epilogue(head_w=o.weight, head_b=o.bias, head_logit=logits[k])
        calls.append(ops.mlp_forward_gather_args(segs, model.input_dim, B, layers, head, dev))
        keep.append((layers, head))

    def run():
        st = ops._lib.raw_stream(dev)
        for args in calls:
            args[-1] = st
            ops.check(lib.rk_mlp_forward_gather(*args), "rk_mlp_forward_gather")
        lg = logits.t()
        return torch.cumprod(torch.sigmoid(lg), dim=1), lg
    run.keep = (segs, keep)
    return run


def measure(kw, B):
    torch.manual_seed(42)
    model = rankops.ESMM(None, vocab_sizes=H.WECHAT_VOCAB, **kw).cuda().eval()
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
    with torch.no_grad():
        prob_a, logit_a = [t.clone() for t in kernel()]
        prob_b, logit_b = torch_forward(model, dense, cat)
        prob_c, logit_c = [t.clone() for t in composed()]
    torch.cuda.synchronize()
    err_b = float(((logit_a - logit_b).abs() / (1 + logit_b.abs())).max())
    err_c = float(((logit_a - logit_c).abs() / (1 + logit_c.abs())).max())
    assert err_b <= 1e-4 and err_c <= 1e-4, f"legs differ: kernel vs torch {err_b}, kernel vs composed {err_c}"
    assert float((prob_a - prob_b).abs().max()) <= 1e-4 and float((prob_a - prob_c).abs().max()) <= 1e-4
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
    r["torch_over_kernel"] = round(med["torch"] / med["kernel"], 2)
    r["composed_over_kernel"] = round(med["composed"] / med["kernel"], 2)
    r["composed_over_kernel_range"] = [round(min(times["composed"]) / max(times["kernel"]), 2),
                                       round(max(times["composed"]) / min(times["kernel"]), 2)]
    r["kernel_vs_torch_max_rel_err"], r["kernel_vs_composed_max_rel_err"] = err_b, err_c
    del graphs, model
    torch.cuda.empty_cache()
    return r


def torch_loss(logits, labels):
    S = torch.cumsum(torch.nn.functional.logsigmoid(logits), dim=1).clamp(max=-1e-7)
    return -(labels * S + (1 - labels) * torch.log1p(-torch.exp(S))).mean(dim=0).sum()


def measure_train(kw, B):
    torch.manual_seed(42)
    engine = rankops.ESMM(None, vocab_sizes=H.WECHAT_VOCAB, trainable=True, **kw).cuda().train()
    torch.manual_seed(42)
    plain = rankops.ESMM(None, vocab_sizes=H.WECHAT_VOCAB, **kw).cuda().train()
    inp = H.to_device(H.dcn_inputs(B, H.WECHAT_VOCAB, 1000), "cuda")
    dense, cat = inp["dense"], inp["category"]
    K = len(engine.task_names)
    y = (torch.rand(B, K, generator=torch.Generator().manual_seed(3)) < 0.5).float()
    labels = torch.cumprod(y, dim=1).cuda()
    opts = {"engine": rankops.Adam(engine.parameters(), lr=1e-3, capturable=True),
            "torch": torch.optim.Adam(plain.parameters(), lr=1e-3, capturable=True)}

    def step_of(model, opt, loss_of, with_opt=True):
        def step():
            with torch.enable_grad():
                for prm in model.parameters():
                    prm.grad = None
                loss_of().backward()
                if with_opt:
                    opt.step()
        return step
    engine_loss = lambda: rankops.esmm_loss(engine(dense, cat)[1], labels)  # noqa: E731
    fns = {"engine": step_of(engine, opts["engine"], engine_loss),
           "torch": step_of(plain, opts["torch"], lambda: torch_loss(torch_forward(plain, dense, cat)[1], labels))}
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
    # after the timing: nothing of the count runs before a capture (forward, loss and backward, no optimizer)
    names = launches_of(step_of(engine, None, engine_loss, with_opt=False))
    r["engine_launches"] = len(names)
    r["engine_launch_list"] = names
    del engine, plain
    torch.cuda.empty_cache()
    return r


def main():
    assert torch.cuda.is_available(), "esmm_time needs a ROCm GPU"
    rankops.load_library()
    result = {"device": torch.cuda.get_device_name(0), "fp32_matrix_peak_tf": FP32_MATRIX_PEAK_TF,
              "sclk_before": shader_clock()}
    batches = (4096, 32768)
    if "--batches" in sys.argv[1:]:
        batches = tuple(int(b) for b in sys.argv[sys.argv.index("--batches") + 1].split(","))
    for shape, kw in SHAPES.items():
        for B in batches:
            r = measure_train(kw, B) if "--train" in sys.argv[1:] else measure(kw, B)
            result[f"{shape}_B{B}"] = r
            print(f"{shape} B {B}: " + ", ".join(f"{k} {v}" for k, v in r.items()), flush=True)
    result["sclk_after"] = shader_clock()
    assert rankops.error_flags() == 0
    print(json.dumps(result))


if __name__ == "__main__":
    main()
