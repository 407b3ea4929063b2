"""Times of the FiBiNET eval forward at B 4096 and 32,768, at the wechat shape (six fields x D 8) with
each bilinear type and at six fields x D 32 (bilinear type "interaction", the widest interaction vector
the one launch takes: 960), three ways, in one process:

  (a) kernel      rk_fibinet_forward, the one launch rankops.FiBiNET runs inside common.fibinet_fits up to one
                  16-sample workgroup per CU (forced here at every batch: two_launch = False)
  (b) torch       the float32 torch-ROCm formulation of the same module (embedding lookups, mean, the
                  SENET nn.Sequential, one einsum per bilinear layer over pre-stacked matrices, the deep
                  layers' modules in eval mode, sigmoid)
  (c) two_launch  rk_fibinet_interaction, then the deep tail (common.tail_launches): what the module
                  runs at larger batches, with `two_launch = True` and outside the one-launch envelope

Every leg is captured in a hipGraph once (after warm calls on a side stream) and timed as replays
between device events; the legs alternate — a, b, c, a, b, c, … — and the median over the rounds is
reported with the fastest and slowest round, whose spread is the noise a ratio has to beat.  The three
are compared with each other before anything is timed.

From the shapes the tool computes the forward's flops per sample (both bilinear layers, the deep layers
and the head) and reports the kernel's rate as a share of the 157.3 TF FP32 matrix peak of the MI355X
(the MFMA FP32 peak, not a measured ceiling; the interaction phase runs on the VALU, the deep layers on
MFMA).  `--batches 2048,8192` measures other batch sizes.  Needs a GPU; prints one JSON line at the end."""
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
from rankops import ops  # noqa: E402

from dien_time import shader_clock  # noqa: E402
from mmoe_time import FP32_MATRIX_PEAK_TF, ROUNDS, replay_us  # noqa: E402

WECHAT = {f: H.WECHAT_VOCAB[f] for f in rankops.deepfm.WECHAT_FIELDS}
D32_FIELDS = {f"field_{i:02d}": 1000 for i in range(6)}
SHAPES = {"wechat_all": (WECHAT, 8, "all"), "wechat_each": (WECHAT, 8, "each"),
          "wechat_interaction": (WECHAT, 8, "interaction"), "d32_interaction": (D32_FIELDS, 32, "interaction")}


def flops_per_sample(model):
    m, D = model.num_categories, model.embedding_dim
    products = m * (m - 1) // 2 if model.bilinear_type == "interaction" else m - 1
    total = 2 * (2 * products * D * D) + 3 * m * (m - 1) * D  # two layers of D x D products; the pair products
    width = model.interaction_width
    for layer in model._tail:
        total += 2 * width * layer.linear.out_features
        width = layer.linear.out_features
    return total + 2 * width + 4


def torch_forward_of(model, cat):
    names = list(model.second_order_embeddings)
    m = model.num_categories
    ij = [(i, j) for i in range(m) for j in range(i + 1, m)]
    dev = cat[names[0]].device
    I = torch.tensor([i for i, _ in ij], device=dev)
    J = torch.tensor([j for _, j in ij], device=dev)

    def stacked(layers):
        w = torch.stack([l.weight.detach() for l in layers])
        if model.bilinear_type == "all":
            w = w.expand(len(ij), -1, -1)
        elif model.bilinear_type == "each":
            w = w[I]
        return w.contiguous()  # one matrix per pair
    We, Wv = stacked(model.bilinear_embedding), stacked(model.bilinear_senet)

    def run():
        linear = torch.cat([model.first_order_embeddings[n](cat[n]) for n in names], dim=1).sum(dim=1, keepdim=True)
        x0 = torch.stack([model.second_order_embeddings[n](cat[n]) for n in names], dim=1)
        a = model.senet(x0.mean(dim=2))
        v = a.unsqueeze(2) * x0
        p = torch.einsum("pdk,bpk->bpd", We, x0[:, I]) * x0[:, J]
        q = torch.einsum("pdk,bpk->bpd", Wv, v[:, I]) * v[:, J]
        h = torch.cat([p.flatten(1), q.flatten(1)], dim=1)
        for layer in model.deep_layers:
            h = layer(h)
        deep = model.deep_output_layer(h)
        total = model.final_layer(torch.cat([linear, deep], dim=1))
        return torch.sigmoid(total), total, linear, deep
    return run


def engine_leg(model, names, idx, two_launch):
    """The module's own bound forward (one launch, or two with two_launch) with its outputs."""
    model.two_launch = two_launch  # (False: the one launch at any batch)
    try:
        built = model._build(names, idx)
    finally:
        model.two_launch = None
    want = "rk_fibinet_interaction" if two_launch else "rk_fibinet_forward"
    assert built.launches[0][0] == want and (two_launch or len(built.launches) == 1), built.launches
    dev = idx[0].device
    out = model._outputs(idx[0].shape[0], dev)

    def run():
        model._run(built, out, ops._lib.raw_stream(dev))
        return out
    run.launches = [n for n, _ in built.launches]
    return run


def measure(shape, B):
    fields, D, bilinear_type = SHAPES[shape]
    torch.manual_seed(42)
    model = rankops.FiBiNET(None, embedding_dim=D, bilinear_type=bilinear_type, vocab_sizes=fields)
    model = H.randomize_eval_stats(model, 43).cuda().eval()
    cat = H.to_device(H.deepfm_inputs(B, fields, 1000)["category"], "cuda")
    names, idx = model._indices(cat)
    fns = {"kernel": engine_leg(model, names, idx, False), "torch": torch_forward_of(model, cat),
           "two_launch": engine_leg(model, names, idx, True)}
    with torch.no_grad():
        outs = {k: [t.clone() for t in fn()] for k, fn in fns.items()}
    torch.cuda.synchronize()

    def err(a, b):
        return max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(a, b))
    err_b, err_c = err(outs["kernel"], outs["torch"]), err(outs["kernel"], outs["two_launch"])
    assert err_b <= 1e-4 and err_c <= 1e-4, f"legs differ: kernel vs torch {err_b}, kernel vs two launches {err_c}"
    graphs = {k: bench.graph_of(fn)[0] for k, fn in fns.items()}
    times = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            times[k].append(replay_us(g))
    r = {"two_launch_list": fns["two_launch"].launches}
    for k, t in times.items():
        r[f"{k}_us"] = {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
    med = {k: statistics.median(t) for k, t in times.items()}
    flops = flops_per_sample(model)
    r["flops_per_sample"] = flops
    r["kernel_tflops"] = round(flops * B / med["kernel"] / 1e6, 2)
    r["share_of_fp32_matrix_peak"] = round(flops * B / med["kernel"] / 1e6 / FP32_MATRIX_PEAK_TF, 4)
    r["torch_over_kernel"] = round(med["torch"] / med["kernel"], 2)
    r["two_launch_over_kernel"] = round(med["two_launch"] / med["kernel"], 2)
    r["two_launch_over_kernel_range"] = [round(min(times["two_launch"]) / max(times["kernel"]), 2),
                                         round(max(times["two_launch"]) / min(times["kernel"]), 2)]
    r["kernel_vs_torch_max_rel_err"], r["kernel_vs_two_launch_max_rel_err"] = err_b, err_c
    del graphs, model
    torch.cuda.empty_cache()
    return r


def main():
    assert torch.cuda.is_available(), "fibinet_time needs a ROCm GPU"
    rankops.load_library()
    result = {"device": torch.cuda.get_device_name(0), "fp32_matrix_peak_tf": FP32_MATRIX_PEAK_TF,
              "sclk_before": shader_clock()}
    batches = (4096, 32768)
    if "--batches" in sys.argv[1:]:
        batches = tuple(int(b) for b in sys.argv[sys.argv.index("--batches") + 1].split(","))
    for shape in SHAPES:
        for B in batches:
            r = measure(shape, B)
            result[f"{shape}_B{B}"] = r
            print(f"{shape} B {B}: " + ", ".join(f"{k} {v}" for k, v in r.items()), flush=True)
    result["sclk_after"] = shader_clock()
    assert rankops.error_flags() == 0
    print(json.dumps(result))


if __name__ == "__main__":
    main()
