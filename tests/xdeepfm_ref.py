"""Restatement of xDeepFM (rankops.XDeepFM's definition: the paper's CIN, Lian et al. 2018 eq. 6-8,
direct form, in the conventions of the reference's DeepFM) in plain torch, in the dtype of its inputs
(the tests run it in float64), plus the seeded inputs and the tolerances of tests/test_gpu_xdeepfm.py.

Tolerances.  A tolerance t is used as |got - ref| <= t * (1 + |ref|) against the float64 restatement
(assert_close with atol = rtol = t).  Each is 50 x the drift of this same restatement run in float32
against float64, drift = max |f32 - f64| / (1 + |f64|) over the seeded inputs of the GPU tests (every
op-level case with both activations for `pooled` and `cin_logit`; the model-level cases for the five
model outputs); 50 x is the margin of the forward-kernel tests (tests/test_train_ops_ref.py) and
covers the MFMA's summation order over K up to 3,840.  tests/test_xdeepfm_ref.py measures the drifts
again and fails if a constant lies outside 25-100 x of what it measures.  Measured on the CPU
(torch 2.x, float32 einsum + matmul):

    pooled                     drift 2.65e-06  ->  POOLED_TOL 1.3e-04
    cin_logit / total_logit    drift 1.46e-06  ->  LOGIT_TOL  7.3e-05   (also linear_logit, deep_logit)
    probability                drift 1.01e-07  ->  PROB_TOL   5.0e-06
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

POOLED_TOL = 1.3e-04
LOGIT_TOL = 7.3e-05
PROB_TOL = 5.0e-06

ACTIVATIONS = ("identity", "relu")

# (name, m fields, D, feature maps per layer, batch): the shapes at which rk_cin_forward takes another
# path (64- or 128-column tiles, padded or unpadded LDS rows, partial sample tiles, widths off the 16
# grid, a sample over several 16-column tiles, K = 3,840)
OP_CASES = [
    ("wechat_b1", 6, 8, (128, 128), 1),
    ("wechat_b7", 6, 8, (128, 128), 7),
    ("wechat_b33", 6, 8, (128, 128), 33),
    ("off_grid", 3, 4, (5, 17, 1), 37),
    ("wide_k", 30, 32, (128, 128), 19),
    ("widest", 2, 16, (256,), 9),
    ("most_fields", 32, 4, (16, 16, 16, 16), 37),
]
ROW_PAD = 8  # the op-level rows lie in a buffer with row stride m * D + ROW_PAD

# model-level cases: (name, fields or None for the wechat tables, D, batch)
WIDE_FIELDS = {f"field_{i:02d}": 1000 for i in range(30)}
MODEL_CASES = [("wechat_b1", None, 8, 1), ("wechat_b300", None, 8, 300), ("wechat_b4096", None, 8, 4096),
               ("wide_b64", WIDE_FIELDS, 32, 64)]


def act_fn(name):
    if name == "identity":
        return lambda x: x
    if name == "relu":
        return torch.relu
    raise ValueError(name)


def cin(x0, Ws, bs, act="identity", chunk=512):
    """x0 [B, m, D]; Ws[k] [H_k, H_{k-1} m] (H_0 = m); bs[k] [H_k] -> pooled [B, sum H_k]."""
    f = act_fn(act)
    out = []
    for s in range(0, x0.shape[0], chunk):
        x = x0[s:s + chunk]
        B, m, D = x.shape
        xk, pooled = x, []
        for W, b in zip(Ws, bs):
            z = (xk.unsqueeze(2) * x.unsqueeze(1)).reshape(B, xk.shape[1] * m, D)  # z[b, h m + i, d]
            xk = f(torch.matmul(W.reshape(W.shape[0], -1), z) + b.view(1, -1, 1))
            pooled.append(xk.sum(dim=2))
        out.append(torch.cat(pooled, dim=1))
    return torch.cat(out, dim=0) if out else x0.new_zeros(0, sum(W.shape[0] for W in Ws))


def deep_layout(p):
    """(Linear index, BatchNorm index or None) of deep_layers, from the state_dict's keys."""
    idx = sorted({int(k.split(".")[1]) for k in p if k.startswith("deep_layers.")})
    lins = [i for i in idx if f"deep_layers.{i}.running_mean" not in p]
    return [(i, i + 1 if f"deep_layers.{i + 1}.running_mean" in p else None) for i in lins]


def forward(p, category, cin_activation="identity", eps=1e-5):
    """(probability, total_logit, linear_logit, cin_logit, deep_logit), each [B, 1], in p's dtype."""
    fields = [k.split(".")[1] for k in p if k.startswith("second_order_embeddings.")]
    first = [p[f"first_order_embeddings.{c}.weight"][category[c]] for c in fields]
    linear = torch.cat(first, dim=1).sum(dim=1, keepdim=True)
    x0 = torch.stack([p[f"second_order_embeddings.{c}.weight"][category[c]] for c in fields], dim=1)
    nl = len([k for k in p if k.startswith("cin_layers.") and k.endswith(".weight")])
    Ws = [p[f"cin_layers.{k}.weight"] for k in range(nl)]
    bs = [p[f"cin_layers.{k}.bias"] for k in range(nl)]
    pooled = cin(x0, Ws, bs, cin_activation)
    cin_logit = F.linear(pooled, p["cin_output_layer.weight"], p["cin_output_layer.bias"])
    h = x0.reshape(x0.shape[0], -1)
    for lin, bn in deep_layout(p):
        h = F.linear(h, p[f"deep_layers.{lin}.weight"], p[f"deep_layers.{lin}.bias"])
        if bn is not None:
            q = f"deep_layers.{bn}."
            h = (h - p[q + "running_mean"]) / torch.sqrt(p[q + "running_var"] + eps) * p[q + "weight"] + p[q + "bias"]
        h = torch.relu(h)
    deep = F.linear(h, p["deep_output_layer.weight"], p["deep_output_layer.bias"])
    total = F.linear(torch.cat([linear, cin_logit, deep], dim=1), p["final_layer.weight"], p["final_layer.bias"])
    return torch.sigmoid(total), total, linear, cin_logit, deep


def floats(p, dtype):
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in p.items()}


# ---------------------------------------------------------------- seeded inputs of the GPU tests

def op_inputs(case, seed=2024):
    """float32 CPU inputs of one op-level case: the row buffer [B, m D + ROW_PAD] (x0 = its first m D
    columns), the layer weights (nn.Conv1d's init range), non-zero biases, and an output layer."""
    _, m, D, maps, B = case
    g = torch.Generator().manual_seed(seed + 131 * m + 17 * D + B + len(maps))
    rows = torch.randn(B, m * D + ROW_PAD, generator=g)
    Ws, bs, hprev = [], [], m
    for h in maps:
        bound = 1.0 / math.sqrt(hprev * m)
        Ws.append((torch.rand(h, hprev * m, generator=g) * 2 - 1) * bound)
        bs.append(torch.rand(h, generator=g) - 0.5 + 0.05)
        hprev = h
    n = sum(maps)
    out_w = (torch.rand(n, generator=g) * 2 - 1) / math.sqrt(n)
    out_b = torch.rand(1, generator=g) - 0.5
    return rows, Ws, bs, out_w, out_b


def op_reference(case, act, dtype=torch.float64):
    """(pooled, cin_logit) of one op-level case from the restatement in `dtype`."""
    _, m, D, _, B = case
    rows, Ws, bs, out_w, out_b = op_inputs(case)
    x0 = rows[:, :m * D].reshape(B, m, D).to(dtype)
    pooled = cin(x0, [w.to(dtype) for w in Ws], [b.to(dtype) for b in bs], act)
    return pooled, pooled @ out_w.to(dtype).view(-1, 1) + out_b.to(dtype)


def build_model(case, seed=42, cin_activation="identity"):
    """Seeded rankops.XDeepFM (CPU, eval, BatchNorm statistics away from their init) of a model case."""
    import helpers as H
    import rankops
    _, fields, D, _ = case
    torch.manual_seed(seed)
    sizes = fields if fields is not None else {f: H.WECHAT_VOCAB[f] for f in rankops.deepfm.WECHAT_FIELDS}
    model = rankops.XDeepFM(None, embedding_dim=D, cin_activation=cin_activation, vocab_sizes=sizes)
    H.randomize_eval_stats(model, seed + 1)
    return model.eval()


def model_inputs(case, seed=1001):
    import helpers as H
    import rankops
    _, fields, _, B = case
    sizes = fields if fields is not None else {f: H.WECHAT_VOCAB[f] for f in rankops.deepfm.WECHAT_FIELDS}
    return H.deepfm_inputs(B, sizes, seed)["category"]


def rel_err(got, ref):
    """max |got - ref| / (1 + |ref|): the quantity the tolerances bound."""
    if ref.numel() == 0:
        return 0.0
    return float(((got.double() - ref.double()).abs() / (1 + ref.double().abs())).max())
