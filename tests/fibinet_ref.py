"""Restatement of FiBiNET (rankops.FiBiNET's definition: SENET field attention and the bilinear
interaction of Huang et al., RecSys 2019, in the conventions of the reference's DeepFM) in plain torch,
in the dtype of its inputs (the tests run it in float64), plus the seeded inputs, the case lists and the
tolerances of tests/test_gpu_fibinet.py.

Tolerances.  rel_err(got, ref) = max |got - ref| / max |ref| is the quantity every tolerance bounds.
Each constant is 50 x the drift of this same restatement run in float32 against float64, drift =
rel_err(f32, f64) over the seeded inputs of the GPU tests (every op-level case with the three bilinear
types for `c` and the attention; the model-level cases for the four model outputs).  The kernels sum in
float32 in their own fixed order (k ascending fmaf chains, the MFMA's order in the deep layers), so
their error is of the restatement's float32 order; 50 x is the margin the other forward-kernel tests
use.  tests/test_fibinet_ref.py measures the drifts again and fails if a constant lies outside
25-100 x of what it measures.  Measured on the CPU (torch 2.x, float32 einsum + matmul):

    c                          drift 3.21e-07  ->  C_TOL     1.6e-05
    attention                  drift 1.61e-07  ->  ATTN_TOL  8.0e-06
    total / linear / deep      drift 5.55e-07  ->  LOGIT_TOL 2.8e-05
    probability                drift 1.02e-07  ->  PROB_TOL  5.1e-06
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

C_TOL = 1.6e-05
ATTN_TOL = 8.0e-06
LOGIT_TOL = 2.8e-05
PROB_TOL = 5.1e-06

BILINEAR_TYPES = ("all", "each", "interaction")

# (name, m fields, D, batch): the shapes at which the two kernels take another path (a partial second
# 16-sample tile, one pair, D off the powers of two, the widest fused interaction vector, just past it,
# 4-sample tiles, the most fields)
OP_CASES = [
    ("wechat_b1", 6, 8, 1),
    ("wechat_b17", 6, 8, 17),
    ("wechat_b33", 6, 8, 33),
    ("two_fields", 2, 4, 5),
    ("off_grid", 7, 12, 37),
    ("widest_fused", 6, 32, 19),
    ("past_fused", 12, 8, 37),
    ("wide", 30, 32, 9),
    ("most_fields", 32, 4, 37),
]
ROW_PAD = 8  # the op-level rows lie in a buffer with row stride m * D + ROW_PAD
REDUCTION_RATIO = 3
# seed of each op-level case: chosen so that the share of exact zeros in the float64 attention lies in
# [0.2, 0.8] (tests/test_fibinet_ref.py checks it): both SENET ReLUs clip, and not everywhere
OP_SEEDS = {"wechat_b1": 0, "wechat_b17": 0, "wechat_b33": 0, "two_fields": 1, "off_grid": 0, "widest_fused": 0,
            "past_fused": 0, "wide": 0, "most_fields": 0}

# model-level cases: (name, fields or None for the wechat tables, D, batch, bilinear type, model kwargs)
D32_FIELDS = {f"field_{i:02d}": 1000 for i in range(6)}
TWELVE_FIELDS = {f"field_{i:02d}": 500 + 37 * i for i in range(12)}
MODEL_CASES = [(f"wechat_b{B}_{t}", None, 8, B, t, {}) for t in BILINEAR_TYPES for B in (1, 300, 4096)] + [
    ("no_bn_b33", None, 8, 33, "interaction", dict(batch_norm=False, hidden_units=[32, 8])),
    ("d32_b64", D32_FIELDS, 32, 64, "interaction", {}),        # the fused path at its widest (960)
    ("twelve_b64", TWELVE_FIELDS, 8, 64, "interaction", {}),   # 1,056 wide: outside the fused envelope
]
MODEL_SEED = 43  # (42 leaves the B = 1 sample without a live attention value)


def reduced(m, ratio=REDUCTION_RATIO):
    return max(1, m // ratio)


def pairs(m):
    return [(i, j) for i in range(m) for j in range(i + 1, m)]


def matrices(m, bilinear_type):
    return {"all": 1, "each": m - 1, "interaction": m * (m - 1) // 2}[bilinear_type]


def bilinear(x, Ws, bilinear_type):
    """x [B, m, D], Ws: the type's list of [D, D] -> [B, P, D]: (W_(i,j) x_i) * x_j over the pairs."""
    m = x.shape[1]
    ij = pairs(m)
    left = torch.stack([x[:, i] for i, _ in ij], dim=1)    # [B, P, D]
    right = torch.stack([x[:, j] for _, j in ij], dim=1)
    if bilinear_type == "all":
        W = Ws[0].unsqueeze(0).expand(len(ij), -1, -1)
    elif bilinear_type == "each":
        W = torch.stack([Ws[i] for i, _ in ij])
    elif bilinear_type == "interaction":
        W = torch.stack(list(Ws))
    else:
        raise ValueError(bilinear_type)
    return torch.einsum("pdk,bpk->bpd", W, left) * right


def interaction(x0, w1, w2, We, Wv, bilinear_type="interaction"):
    """x0 [B, m, D], w1 [r, m], w2 [m, r], We / Wv lists of [D, D] -> (c [B, m (m - 1) D], a [B, m])."""
    z = x0.mean(dim=2)
    a = torch.relu(F.linear(torch.relu(F.linear(z, w1)), w2))
    v = a.unsqueeze(2) * x0
    p = bilinear(x0, We, bilinear_type)
    q = bilinear(v, Wv, bilinear_type)
    B = x0.shape[0]
    return torch.cat([p.reshape(B, -1), q.reshape(B, -1)], dim=1), a


def deep_layout(p):
    """(Linear index, BatchNorm index or None) of deep_layers, from the state_dict's keys."""
    idx = sorted({int(k.split(".")[1]) for k in p if k.startswith("deep_layers.")})
    lins = [i for i in idx if f"deep_layers.{i}.running_mean" not in p]
    return [(i, i + 1 if f"deep_layers.{i + 1}.running_mean" in p else None) for i in lins]


def bilinear_type_of(p):
    """The bilinear type from the number of matrices (with two fields the three types coincide)."""
    m = len([k for k in p if k.startswith("second_order_embeddings.")])
    n = len([k for k in p if k.startswith("bilinear_embedding.")])
    return "all" if n == 1 else "each" if n == m - 1 else "interaction"


def attention(p, category):
    """The SENET attention a [B, m] of a model's parameters over these indices."""
    fields = [k.split(".")[1] for k in p if k.startswith("second_order_embeddings.")]
    x0 = torch.stack([p[f"second_order_embeddings.{c}.weight"][category[c]] for c in fields], dim=1)
    return torch.relu(F.linear(torch.relu(F.linear(x0.mean(dim=2), p["senet.0.weight"])), p["senet.2.weight"]))


def forward(p, category, bilinear_type=None, eps=1e-5):
    """(probability, total_logit, linear_logit, deep_logit), each [B, 1], in p's dtype."""
    fields = [k.split(".")[1] for k in p if k.startswith("second_order_embeddings.")]
    if bilinear_type is None:
        bilinear_type = bilinear_type_of(p)
    first = [p[f"first_order_embeddings.{c}.weight"][category[c]] for c in fields]
    linear = torch.cat(first, dim=1).sum(dim=1, keepdim=True)
    x0 = torch.stack([p[f"second_order_embeddings.{c}.weight"][category[c]] for c in fields], dim=1)
    n = matrices(len(fields), bilinear_type)
    We = [p[f"bilinear_embedding.{k}.weight"] for k in range(n)]
    Wv = [p[f"bilinear_senet.{k}.weight"] for k in range(n)]
    h, _ = interaction(x0, p["senet.0.weight"], p["senet.2.weight"], We, Wv, bilinear_type)
    for lin, bn in deep_layout(p):
        h = F.linear(h, p[f"deep_layers.{lin}.weight"], p[f"deep_layers.{lin}.bias"])
        if bn is not None:
            q = f"deep_layers.{bn}."
            h = (h - p[q + "running_mean"]) / torch.sqrt(p[q + "running_var"] + eps) * p[q + "weight"] + p[q + "bias"]
        h = torch.relu(h)
    deep = F.linear(h, p["deep_output_layer.weight"], p["deep_output_layer.bias"])
    total = F.linear(torch.cat([linear, deep], dim=1), p["final_layer.weight"], p["final_layer.bias"])
    return torch.sigmoid(total), total, linear, deep


def floats(p, dtype):
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in p.items()}


# ---------------------------------------------------------------- seeded inputs of the GPU tests

def _uniform(g, shape, fan_in):
    """nn.Linear's default init: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))."""
    return (torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(fan_in)


def op_inputs(case, bilinear_type="interaction", seed=None):
    """float32 CPU inputs of one op-level case: the row buffer [B, m D + ROW_PAD] of N(0, 1) values (x0 =
    its first m D columns), the SENET weights and the two lists of bilinear matrices (nn.Linear's default
    init).  Rows and SENET weights do not depend on the bilinear type."""
    name, m, D, B = case
    seed = OP_SEEDS[name] if seed is None else seed
    g = torch.Generator().manual_seed(1000 * seed + 131 * m + 17 * D + B)
    rows = torch.randn(B, m * D + ROW_PAD, generator=g)
    r = reduced(m)
    w1, w2 = _uniform(g, (r, m), m), _uniform(g, (m, r), r)
    n = matrices(m, bilinear_type)
    We = [_uniform(g, (D, D), D) for _ in range(n)]
    Wv = [_uniform(g, (D, D), D) for _ in range(n)]
    return rows, w1, w2, We, Wv


def op_reference(case, bilinear_type, dtype=torch.float64):
    """(c, a) of one op-level case from the restatement in `dtype`."""
    _, m, D, B = case
    rows, w1, w2, We, Wv = op_inputs(case, bilinear_type)
    x0 = rows[:, :m * D].reshape(B, m, D).to(dtype)
    return interaction(x0, w1.to(dtype), w2.to(dtype), [w.to(dtype) for w in We], [w.to(dtype) for w in Wv],
                       bilinear_type)


def case_sizes(case):
    import helpers as H
    import rankops
    fields = case[1]
    return fields if fields is not None else {f: H.WECHAT_VOCAB[f] for f in rankops.deepfm.WECHAT_FIELDS}


def build_model(case, seed=MODEL_SEED):
    """Seeded rankops.FiBiNET (CPU, eval, BatchNorm statistics away from their init) of a model case."""
    import helpers as H
    import rankops
    _, _, D, _, bilinear_type, kw = case
    torch.manual_seed(seed)
    model = rankops.FiBiNET(None, embedding_dim=D, bilinear_type=bilinear_type, vocab_sizes=case_sizes(case), **kw)
    H.randomize_eval_stats(model, seed + 1)
    return model.eval()


def model_inputs(case, seed=1001):
    import helpers as H
    return H.deepfm_inputs(case[3], case_sizes(case), seed)["category"]


def rel_err(got, ref):
    """max |got - ref| / max |ref|: the quantity the tolerances bound."""
    if ref.numel() == 0:
        return 0.0
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300))
