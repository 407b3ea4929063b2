"""Restatement of MMoE (rankops.MMoE's definition: Ma et al., KDD 2018, in the conventions of the
reference's DCN) in plain torch matmul / softmax / einsum, in the dtype of its inputs (the tests run it
in float64), plus the seeded inputs and the tolerances of tests/test_gpu_mmoe.py.

Tolerances.  A tolerance t is used as |got - ref| <= t * (1 + |ref|) against the float64 restatement
(`rel_err`).  Each is 50 x the drift of this same restatement run in float32 against float64,
drift = max |f32 - f64| / (1 + |f64|) over the seeded inputs of the GPU tests: every ordinary op-level
case for the four op outputs, plus the model-level cases for logits and probabilities.  The
`extreme_gate` case (gate weights x 400, logits of magnitude ~100 whose float32 rounding moves the
near-one-hot softmax) has its own constants from its own drift, so that it does not loosen the others.
tests/test_mmoe_ref.py measures the drifts again and fails if a constant lies outside 25-100 x of what
it measures.  The float32 run takes every sum in a fixed order with element-wise operations
(`ordered=True`, see `linear`): torch's float32 matmul sums in an order that depends on the machine,
and with it the extreme case's drift came out 1.7e-6 on one CPU and 3.7e-7 on another, too far apart for
one constant to sit inside both bands.  Measured (torch 2.x, CPU):

    ordinary   mixed  drift 3.44e-07  ->  MIXED_TOL 1.7e-05
               gates  drift 2.48e-07  ->  GATE_TOL  1.2e-05
               logits drift 1.66e-07  ->  LOGIT_TOL 8.3e-06
               probs  drift 4.28e-08  ->  PROB_TOL  2.1e-06
    extreme    mixed  drift 1.29e-06  ->  EXTREME_MIXED_TOL 6.5e-05
               gates  drift 1.24e-06  ->  EXTREME_GATE_TOL  6.2e-05
               logits drift 6.38e-08  ->  EXTREME_LOGIT_TOL 3.2e-06
               probs  drift 3.19e-08  ->  EXTREME_PROB_TOL  1.6e-06
"""
from __future__ import annotations

import math

import torch

MIXED_TOL = 1.7e-05
GATE_TOL = 1.2e-05
LOGIT_TOL = 8.3e-06
PROB_TOL = 2.1e-06
EXTREME_MIXED_TOL = 6.5e-05
EXTREME_GATE_TOL = 6.2e-05
EXTREME_LOGIT_TOL = 3.2e-06
EXTREME_PROB_TOL = 1.6e-06

# (name, width, E, K, expert units, tower units, B): the smallest shapes at which rk_mmoe_forward can
# still go wrong (the default shape with a ragged last tile, one live row, 16 + 1 rows, widths off the
# 16 grid with no tower layer and one expert layer, the deepest stacks over an odd input width, a
# single expert (gate = 1), K E = 64 with the 512-wide two-tile path, near-one-hot gates)
OP_CASES = [
    ("wechat", 50, 4, 3, (256, 128), (64,), 300),
    ("one_row", 50, 4, 3, (256, 128), (64,), 1),
    ("tile_edge", 50, 2, 2, (64,), (16,), 17),
    ("odd", 50, 3, 2, (24,), (), 33),
    ("deep", 37, 8, 4, (100, 40, 24), (20, 7), 40),
    ("one_expert", 50, 1, 1, (16,), (8,), 20),
    ("wide", 200, 16, 4, (512,), (512,), 16),
    ("extreme_gate", 50, 4, 3, (32,), (8,), 64),
]
EXTREME = "extreme_gate"
ROW_PAD = 6       # the op-level rows lie in a buffer with row stride width + ROW_PAD
X_STD = 0.7       # spread of the op-level input rows
GATE_SCALE = 3.0  # ordinary cases: gate weights and biases at 3 x nn.Linear's init range, so that the gates
                  # are neither uniform nor one-hot (the bands test_mmoe_ref.py asserts)
EXTREME_GATE_SCALE = 400.0

# model-level cases: (name, vocab ("small" | "wechat"), batch, constructor arguments)
ALT_CONFIG = dict(num_experts=8, expert_hidden_units=(64,), tower_hidden_units=(), task_names=("read_comment", "like"))
MODEL_CASES = [
    ("small_default", "small", 300, {}),
    ("small_alt", "small", 300, ALT_CONFIG),
    ("wechat_default", "wechat", 257, {}),
    ("wechat_alt", "wechat", 257, ALT_CONFIG),
]


def case(name):
    return next(c for c in OP_CASES if c[0] == name)


def tolerances(name):
    """(mixed, gates, logits, probs) tolerances of an op-level case."""
    if name == EXTREME:
        return EXTREME_MIXED_TOL, EXTREME_GATE_TOL, EXTREME_LOGIT_TOL, EXTREME_PROB_TOL
    return MIXED_TOL, GATE_TOL, LOGIT_TOL, PROB_TOL


# ---------------------------------------------------------------- the definition

def linear(x, W, b=None, ordered=False):
    """x W^T + b.  ordered: the sum over the input columns taken one column at a time, each product and
    each addition rounded on its own (element-wise torch ops), instead of torch's matmul, whose float32
    summation order depends on the machine's vector width and thread count.  The float32 drift the
    tolerances come from is measured this way, so that it is the same number on every machine."""
    if ordered:
        z = torch.zeros(x.shape[0], W.shape[0], dtype=x.dtype)
        for j in range(W.shape[1]):
            z += x[:, j:j + 1] * W[:, j].unsqueeze(0)
    else:
        z = x @ W.t()
    return z if b is None else z + b


def stack(x, layers, clipped=None, ordered=False):
    """Linear + ReLU per (W, b); b may be None.  `clipped` collects each layer's share of negative
    pre-activations."""
    for W, b in layers:
        z = linear(x, W, b, ordered)
        if clipped is not None:
            clipped.append(float((z < 0).double().mean()))
        x = torch.relu(z)
    return x


def mmoe(x, experts, gates, towers=None, clipped=None, ordered=False):
    """x [B, width]; experts: E lists of (W, b); gates: K (W [E, width], b); towers: K (hidden [(W, b)…],
    (w_out [1, ·], b_out)).  Returns (mixed [B, K, H], gate_probs [B, K, E]) and, with towers,
    (logits [B, K], probs [B, K]).  ordered: every sum in a fixed order (see linear)."""
    f = torch.stack([stack(x, layers, clipped, ordered) for layers in experts], dim=1)        # [B, E, H]
    if ordered:
        g = []
        for W, b in gates:
            z = linear(x, W, b, True)
            ex = torch.exp(z - z.max(dim=1, keepdim=True).values)
            total = torch.zeros(x.shape[0], 1, dtype=x.dtype)
            for e in range(ex.shape[1]):
                total += ex[:, e:e + 1]
            g.append(ex / total)
        g = torch.stack(g, dim=1)                                                             # [B, K, E]
        m = torch.zeros(x.shape[0], g.shape[1], f.shape[2], dtype=x.dtype)
        for e in range(f.shape[1]):
            m += g[:, :, e:e + 1] * f[:, e:e + 1, :]
    else:
        g = torch.stack([torch.softmax(linear(x, W, b), dim=1) for W, b in gates], dim=1)
        m = torch.einsum("bke,beh->bkh", g, f)                                                # [B, K, H]
    if towers is None:
        return m, g
    logits = []
    for k, (hidden, (w_out, b_out)) in enumerate(towers):
        t = stack(m[:, k], hidden, clipped, ordered)
        logits.append(linear(t, w_out.reshape(1, -1), b_out.reshape(1, 1), ordered))
    logits = torch.cat(logits, dim=1)
    return m, g, logits, torch.sigmoid(logits)


def _layout(p, prefix):
    """{stack index: [Linear indices]} of a ModuleList of Sequentials, from the state_dict's keys."""
    out = {}
    for k in p:
        if k.startswith(prefix) and k.endswith(".weight"):
            _, s, i, _ = k.split(".")
            out.setdefault(int(s), []).append(int(i))
    return {s: sorted(v) for s, v in out.items()}


def model_parts(p):
    """(experts, gates, towers) of a rankops.MMoE state_dict, in mmoe()'s form."""
    ex = _layout(p, "experts.")
    experts = [[(p[f"experts.{e}.{i}.weight"], p[f"experts.{e}.{i}.bias"]) for i in ex[e]] for e in sorted(ex)]
    K = len([k for k in p if k.startswith("gates.") and k.endswith(".weight")])
    gates = [(p[f"gates.{k}.weight"], p[f"gates.{k}.bias"]) for k in range(K)]
    tw = _layout(p, "towers.")
    towers = [([(p[f"towers.{k}.{i}.weight"], p[f"towers.{k}.{i}.bias"]) for i in tw.get(k, [])],
               (p[f"tower_outputs.{k}.weight"], p[f"tower_outputs.{k}.bias"])) for k in range(K)]
    return experts, gates, towers


def model_row(p, dense, category, keep=None):
    """x = cat[dense, embeddings…].  keep: {field: [B] mask}; where it is 0 the field's columns are zero
    (what the engine gathers for an out-of-range id) and the id is not looked up."""
    keep = keep or {}
    fields = [k.split(".")[1] for k in p if k.startswith("embeddings.")]
    cols = [dense.to(p[f"embeddings.{fields[0]}.weight"].dtype)]
    for c in fields:
        w = p[f"embeddings.{c}.weight"]
        if c in keep:
            cols.append(w[category[c].clamp(0, w.shape[0] - 1)] * keep[c].to(w.dtype).unsqueeze(1))
        else:
            cols.append(w[category[c]])
    return torch.cat(cols, dim=1)


def forward(p, dense, category, keep=None, ordered=False):
    """(probabilities [B, K], logits [B, K]) of a rankops.MMoE state_dict, in p's dtype."""
    x = model_row(p, dense, category, keep)
    experts, gates, towers = model_parts(p)
    _, _, logits, probs = mmoe(x, experts, gates, towers, ordered=ordered)
    return probs, logits


def floats(p, dtype):
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in p.items()}


def cast(obj, dtype):
    if isinstance(obj, torch.Tensor):
        return obj.to(dtype)
    if isinstance(obj, (list, tuple)):
        return type(obj)(cast(o, dtype) for o in obj)
    return obj


# ---------------------------------------------------------------- seeded inputs of the GPU tests

def _linear(g, n, k, scale=1.0):
    """nn.Linear's init range: W and b uniform in +-1/sqrt(k)."""
    bound = scale / math.sqrt(k)
    return (torch.rand(n, k, generator=g) * 2 - 1) * bound, (torch.rand(n, generator=g) * 2 - 1) * bound


def _stack_inputs(g, k, units):
    layers = []
    for n in units:
        layers.append(_linear(g, n, k))
        k = n
    return layers, k


# Seeds chosen so that a case sits inside the gate bands of tests/test_mmoe_ref.py (two experts over 34
# (row, task) pairs: the band for the mean largest gate is 0.75-0.85, and seed 2025 gives 0.746)
CASE_SEEDS = {"tile_edge": 2036}


def op_inputs(c, seed=None):
    """float32 CPU inputs of one op-level case: the row buffer [B, width + ROW_PAD] (x = its first `width`
    columns), experts, gates and towers in mmoe()'s form."""
    name, width, E, K, eu, tu, B = c
    seed = CASE_SEEDS.get(name, 2025) if seed is None else seed
    g = torch.Generator().manual_seed(seed + 131 * width + 17 * E + 7 * K + B + len(eu) + 3 * len(tu))
    rows = torch.randn(B, width + ROW_PAD, generator=g) * X_STD
    experts, H = [], None
    for _ in range(E):
        layers, H = _stack_inputs(g, width, eu)
        experts.append(layers)
    scale = EXTREME_GATE_SCALE if name == EXTREME else GATE_SCALE
    gates = [_linear(g, E, width, scale) for _ in range(K)]
    towers = []
    for _ in range(K):
        hidden, last = _stack_inputs(g, H, tu)
        w, b = _linear(g, 1, last)
        towers.append((hidden, (w, b)))
    return rows, experts, gates, towers


_REFS = {}


def op_reference(c, dtype=torch.float64, clipped=None, ordered=False):
    """(mixed, gate_probs, logits, probs) of one op-level case from the restatement in `dtype`; the float64
    result is computed once and shared (do not modify it)."""
    key = (c[0], dtype, ordered)
    if clipped is None and key in _REFS:
        return _REFS[key]
    rows, experts, gates, towers = op_inputs(c)
    out = mmoe(rows[:, :c[1]].to(dtype), cast(experts, dtype), cast(gates, dtype), cast(towers, dtype), clipped,
               ordered)
    if clipped is None:
        _REFS[key] = out
    return out


def vocab(which):
    import helpers as H
    return H.SMALL_VOCAB if which == "small" else H.WECHAT_VOCAB


def build_model(mc, seed=42):
    """Seeded rankops.MMoE (CPU, eval) of a model case, its gate weights and biases x GATE_SCALE."""
    import rankops
    _, which, _, kw = mc
    torch.manual_seed(seed)
    model = rankops.MMoE(None, vocab_sizes=vocab(which), **kw)
    with torch.no_grad():
        for gate in model.gates:
            gate.weight.mul_(GATE_SCALE)
            gate.bias.mul_(GATE_SCALE)
    return model.eval()


def model_inputs(mc, seed=1000):
    import helpers as H
    _, which, B, _ = mc
    return H.dcn_inputs(B, vocab(which), seed)


def rel_err(got, ref):
    """max |got - ref| / (1 + |ref|): the quantity the tolerances bound."""
    if ref.numel() == 0:
        return 0.0
    return float(((got.double().cpu() - ref.double()).abs() / (1 + ref.double().abs())).max())
