"""Times of xDeepFM's CIN kernel (rk_cin_forward) and of the whole prepared forward
(XDeepFM.prepare's run(): rk_cin_forward + the deep tail), at B 4096 and 32,768, for the wechat shape
(6 fields, D 8, maps 128-128) and the 30-field x D 32 shape (maps 128-128), in one process.

Every time is from device events around warmed repeats.  The kernel leg (the launch with only
cin_logit asked for: gather, CIN layers, pooling, output layer) is alternated, in the same call, with
the float32 torch-ROCm restatement of the CIN on the same rows (tests/xdeepfm_ref.cin: the outer
product materialised, one matmul per layer, pooled, then the output layer) — kernel, torch, kernel,
torch — and both rounds are printed: their spread is the noise the comparison has to beat.  The two
are compared before anything is timed.

From the shapes the tool computes the CIN's flops, 2 D sum_k H_k H_{k-1} m per sample, and reports
the kernel's rate as a share of the 157.3 TF FP32 matrix peak of the MI355X (the MFMA FP32 peak, not
a measured ceiling).  `--batches 2048,8192` measures other batch sizes.  Needs a GPU; prints one JSON
line at the end.

The training leg (`train_*` keys; `--no-train` skips it) times one whole step at the same four points:
XDeepFM(trainable=True) train forward + BCE + backward + rankops.Adam, eager and as a replayed hipGraph,
alternated with the float32 torch restatement of the model (the same modules, the CIN as
tests/xdeepfm_ref.cin with the outer product materialised) under torch autograd with torch.optim.Adam,
on the same rows, in the same process.  The first step's loss of the two is compared before timing."""
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402,F401  (sets sys.path for rankops and tests/)
import torch  # noqa: E402

import helpers as H  # noqa: E402
import rankops  # noqa: E402
import xdeepfm_ref as X  # noqa: E402
from rankops import common, ops  # noqa: E402

from dien_time import shader_clock  # noqa: E402

FP32_MATRIX_PEAK_TF = 157.3
ROUNDS = 2
SHAPES = {"wechat_6x8": (None, 8), "wide_30x32": (X.WIDE_FIELDS, 32)}


def event_us(fn, iters):
    """Device time of one call of fn: events around `iters` calls after two warm ones."""
    fn()
    fn()
    st = torch.cuda.current_stream()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(st)
    for _ in range(iters):
        fn()
    end.record(st)
    end.synchronize()
    return 1e3 * start.elapsed_time(end) / iters


def cin_flops(m, D, maps):
    total, hprev = 0, m
    for h in maps:
        total += 2 * D * h * hprev * m
        hprev = h
    return total


def measure(fields, D, B):
    case = ("time", fields, D, B)
    model = X.build_model(case).cuda()
    cat = H.to_device(X.model_inputs(case), "cuda")
    names = list(model.second_order_embeddings)
    m, maps = model.num_categories, model.cin_layer_sizes
    dev = torch.device("cuda", torch.cuda.current_device())
    second = [ops.table_segment(model.second_order_embeddings[n].weight, cat[n], f * D) for f, n in enumerate(names)]
    images = [common.CIN_PACKED(c.weight) for c in model.cin_layers]
    biases = [c.bias for c in model.cin_layers]
    logit = torch.empty(B, 1, device=dev)
    args, _keep = ops.cin_forward_args(second, None, D, B, images, biases, maps, model.cin_activation,
                                       model.cin_output_layer.weight, model.cin_output_layer.bias, None, None, None,
                                       logit, dev)
    args[-1] = ops._lib.raw_stream(dev)
    fn = ops._lib.load().rk_cin_forward

    def kernel():
        ops.check(fn(*args), "rk_cin_forward")

    with torch.no_grad():
        x0 = torch.stack([model.second_order_embeddings[n].weight[cat[n]] for n in names], dim=1).contiguous()
        Ws = [c.weight.detach().reshape(c.weight.shape[0], -1) for c in model.cin_layers]
        bs = [c.bias.detach() for c in model.cin_layers]
        ow, ob = model.cin_output_layer.weight.detach(), model.cin_output_layer.bias.detach()

    def torch_cin():
        with torch.no_grad():
            return torch.nn.functional.linear(X.cin(x0, Ws, bs, model.cin_activation, chunk=B), ow, ob)

    kernel()
    want = torch_cin()
    torch.cuda.synchronize()
    err = X.rel_err(logit.cpu(), want.cpu())
    assert err <= X.LOGIT_TOL, f"kernel and torch restatement differ: {err}"
    run = model.prepare(cat)
    iters = 20 if B * m * D <= 4096 * 960 else 4
    legs = {"cin_kernel_us": lambda: event_us(kernel, iters), "torch_cin_us": lambda: event_us(torch_cin, iters),
            "prepared_forward_us": lambda: event_us(run, iters)}
    r = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, leg in legs.items():
            r[k].append(round(leg(), 2))
    flops = cin_flops(m, D, maps)
    best = min(r["cin_kernel_us"])
    r["cin_flops_per_sample"] = flops
    r["cin_tflops"] = round(flops * B / best / 1e6, 2)
    r["share_of_fp32_matrix_peak"] = round(flops * B / best / 1e6 / FP32_MATRIX_PEAK_TF, 4)
    r["kernel_vs_torch"] = round(min(r["torch_cin_us"]) / best, 2)
    r["kernel_torch_max_rel_err"] = err
    del x0, want
    torch.cuda.empty_cache()
    return r


class TorchXDeepFM(torch.nn.Module):
    """The float32 torch restatement of a rankops.XDeepFM for the training baseline: a deep copy of
    its modules run by torch (embeddings, tests/xdeepfm_ref.cin, the deep layers as they are)."""

    def __init__(self, model):
        super().__init__()
        self.m = copy.deepcopy(model)

    def forward(self, cat):
        m = self.m
        names = list(m.second_order_embeddings)
        linear = torch.cat([m.first_order_embeddings[n](cat[n]) for n in names], dim=1).sum(dim=1, keepdim=True)
        x0 = torch.stack([m.second_order_embeddings[n](cat[n]) for n in names], dim=1)
        pooled = X.cin(x0, [c.weight for c in m.cin_layers], [c.bias for c in m.cin_layers], m.cin_activation,
                       chunk=x0.shape[0])
        cin_logit = m.cin_output_layer(pooled)
        h = x0.reshape(x0.shape[0], -1)
        for layer in m.deep_layers:
            h = layer(h)
        deep = m.deep_output_layer(h)
        return torch.sigmoid(m.final_layer(torch.cat([linear, cin_logit, deep], dim=1)))


def measure_train(fields, D, B):
    case = ("time", fields, D, B)
    sizes = fields if fields is not None else {f: H.WECHAT_VOCAB[f] for f in rankops.deepfm.WECHAT_FIELDS}
    torch.manual_seed(42)
    model = rankops.XDeepFM(None, embedding_dim=D, vocab_sizes=sizes, dropout_rate=0.0, trainable=True).cuda().train()
    twin = TorchXDeepFM(model).cuda().train()  # dropout off on both sides: one loss to compare
    cat = H.to_device(X.model_inputs(case), "cuda")
    label = (torch.rand(B, generator=torch.Generator().manual_seed(5)) < 0.3).float().cuda()
    crit = torch.nn.BCELoss()
    opt = rankops.Adam(model.parameters(), lr=1e-3, capturable=True)
    topt = torch.optim.Adam(twin.parameters(), lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = crit(model(cat)[0].squeeze(1), label)
        loss.backward()
        opt.step()
        return loss

    def torch_step():
        topt.zero_grad(set_to_none=True)
        loss = crit(twin(cat).squeeze(1), label)
        loss.backward()
        topt.step()
        return loss

    a, b = float(step().detach()), float(torch_step().detach())
    assert abs(a - b) <= 1e-4 * (1 + abs(b)), f"first-step loss: engine {a}, torch {b}"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        step()
    iters = 10 if B * len(sizes) * D <= 4096 * 960 else 3
    legs = {"train_step_eager_us": lambda: event_us(step, iters), "train_step_graph_us": lambda: event_us(graph.replay, iters),
            "train_step_torch_us": lambda: event_us(torch_step, iters)}
    r = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, leg in legs.items():
            r[k].append(round(leg(), 1))
    r["train_torch_vs_graph"] = round(min(r["train_step_torch_us"]) / min(r["train_step_graph_us"]), 2)
    r["train_torch_vs_eager"] = round(min(r["train_step_torch_us"]) / min(r["train_step_eager_us"]), 2)
    r["train_first_loss"] = [a, b]
    del graph, model, twin, opt, topt
    torch.cuda.empty_cache()
    return r


def main():
    assert torch.cuda.is_available(), "xdeepfm_time needs a ROCm GPU"
    rankops.load_library()
    result = {"device": torch.cuda.get_device_name(0), "fp32_matrix_peak_tf": FP32_MATRIX_PEAK_TF,
              "sclk_before": shader_clock()}
    batches = (4096, 32768)
    if "--batches" in sys.argv[1:]:
        batches = tuple(int(b) for b in sys.argv[sys.argv.index("--batches") + 1].split(","))
    for name, (fields, D) in SHAPES.items():
        for B in batches:
            r = measure(fields, D, B)
            if "--no-train" not in sys.argv[1:]:
                r.update(measure_train(fields, D, B))
            result[f"{name}_B{B}"] = r
            print(f"{name} B {B}: " + ", ".join(f"{k} {v}" for k, v in r.items()), flush=True)
    result["sclk_after"] = shader_clock()
    assert rankops.error_flags() == 0
    print(json.dumps(result))


if __name__ == "__main__":
    main()
