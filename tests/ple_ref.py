"""Restatement of PLE (rankops.PLE's definition: Tang et al., RecSys 2020, in the conventions of
rankops.MMoE and the reference's DCN) in plain torch matmul / softmax / einsum, in the dtype of its inputs
(the tests run it in float64), plus the seeded inputs and the tolerances of tests/test_gpu_ple.py.  The
Linear + ReLU stacks, the fixed-order sums and the embedding row are tests/mmoe_ref.py's.

Tolerances.  A tolerance t is used as |got - ref| <= t * (1 + |ref|) against the float64 restatement
(`rel_err`).  Each is 50 x the drift of this same restatement run in float32 against float64,
drift = max |f32 - f64| / (1 + |f64|) over the seeded inputs of the GPU tests: every ordinary op-level case
for the representations and gates of every level, the logits and the probabilities, plus the model-level
cases for logits and probabilities.  The `extreme_gate` case (gate weights x 400, near-one-hot softmax) has
its own constants from its own drift, so that it does not loosen the others.  tests/test_ple_ref.py
measures the drifts again and fails if a constant lies outside 25-100 x of what it measures.  The float32
run takes every sum in a fixed order with element-wise operations (`ordered=True`, mmoe_ref.linear), so the
figures do not depend on the host's matmul.  Measured (torch 2.x, CPU):

    ordinary   reps   drift 5.68e-07  ->  REP_TOL   2.8e-05
               gates  drift 4.10e-07  ->  GATE_TOL  2.1e-05
               logits drift 1.66e-07  ->  LOGIT_TOL 8.3e-06
               probs  drift 5.46e-08  ->  PROB_TOL  2.7e-06
    extreme    reps   drift 7.30e-06  ->  EXTREME_REP_TOL   3.6e-04
               gates  drift 4.82e-06  ->  EXTREME_GATE_TOL  2.4e-04
               logits drift 1.07e-06  ->  EXTREME_LOGIT_TOL 5.3e-05
               probs  drift 1.86e-07  ->  EXTREME_PROB_TOL  9.3e-06
"""
from __future__ import annotations

import torch

from mmoe_ref import ROW_PAD, X_STD, _linear, cast, floats, linear, model_row, rel_err, stack, vocab  # noqa: F401

REP_TOL = 2.8e-05
GATE_TOL = 2.1e-05
LOGIT_TOL = 8.3e-06
PROB_TOL = 2.7e-06
EXTREME_REP_TOL = 3.6e-04
EXTREME_GATE_TOL = 2.4e-04
EXTREME_LOGIT_TOL = 5.3e-05
EXTREME_PROB_TOL = 9.3e-06

# (name, width, L, K, ms, mc, expert units, tower units, B): the smallest shapes at which rk_ple_forward
# can still go wrong (the default shape with a ragged last tile, one live row, L = 1 and ms = 0 (MMoE), 16 + 1
# rows, widths off the 16 grid with no tower layer over three levels, the deepest stacks over an odd input
# width, a single task, the widest configuration common.ple_fits accepts — 512-wide layers and a 320-wide
# representation on the two-tile path, 159,104 of the 163,840 B of LDS —, near-one-hot gates)
OP_CASES = [
    ("wechat", 50, 2, 3, 2, 2, (256, 128), (64,), 300),
    ("one_row", 50, 2, 3, 2, 2, (256, 128), (64,), 1),
    ("mmoe_like", 50, 1, 3, 0, 4, (256, 128), (64,), 33),
    ("tile_edge", 50, 2, 2, 1, 1, (64,), (16,), 17),
    ("odd", 37, 3, 2, 2, 1, (24,), (), 33),
    ("deep", 37, 2, 4, 1, 3, (100, 40, 24), (20, 7), 40),
    ("one_task", 50, 2, 1, 2, 1, (16,), (8,), 20),
    ("corner", 200, 2, 1, 1, 2, (512, 320), (512,), 16),
    ("extreme_gate", 50, 2, 3, 2, 2, (32,), (8,), 64),
]
EXTREME = "extreme_gate"
GATE_SCALE = 3.0  # ordinary cases: gate weights and biases at 3 x nn.Linear's init range, so that the gates
                  # are neither uniform nor one-hot (the bands test_ple_ref.py asserts)
DEEP_GATE_SCALE = 8.0   # the same for the gates of levels >= 1: their inputs are mixtures of ReLU outputs, smaller
                        # than the rows and alike from row to row, and at 3 x these gates were near uniform
EXTREME_GATE_SCALE = 400.0
WEIGHT_SCALE = 2.0  # expert and tower layers at 2 x nn.Linear's init range: at 1 x a Linear + ReLU passes on ~0.4 of
                    # its input's spread, and through L levels of up to three layers the logits carried too
                    # little of the shared path for the perturbations of test_ple_ref.py to show

# model-level cases: (name, vocab ("small" | "wechat"), batch, constructor arguments)
ALT_CONFIG = dict(num_levels=3, num_specific_experts=1, num_shared_experts=2, expert_hidden_units=(64,),
                  tower_hidden_units=(), task_names=("read_comment", "like"))
MODEL_CASES = [
    ("small_default", "small", 300, {}),
    ("small_alt", "small", 300, ALT_CONFIG),
    ("wechat_default", "wechat", 257, {}),
    ("wechat_alt", "wechat", 257, ALT_CONFIG),
]


def case(name):
    return next(c for c in OP_CASES if c[0] == name)


def tolerances(name):
    """(representations, gates, logits, probs) tolerances of an op-level case."""
    if name == EXTREME:
        return EXTREME_REP_TOL, EXTREME_GATE_TOL, EXTREME_LOGIT_TOL, EXTREME_PROB_TOL
    return REP_TOL, GATE_TOL, LOGIT_TOL, PROB_TOL


# ---------------------------------------------------------------- the definition

def gate(x, wb, ordered=False):
    """softmax(x W^T + b) over the columns, the maximum subtracted."""
    z = linear(x, wb[0], wb[1], ordered)
    if not ordered:
        return torch.softmax(z, dim=1)
    ex = torch.exp(z - z.max(dim=1, keepdim=True).values)
    total = torch.zeros(x.shape[0], 1, dtype=x.dtype)
    for c in range(ex.shape[1]):
        total += ex[:, c:c + 1]
    return ex / total


def mix(g, outputs, ordered=False):
    """sum_c g[:, c] * outputs[c], c ascending."""
    if ordered:
        m = torch.zeros_like(outputs[0])
        for c, f in enumerate(outputs):
            m += g[:, c:c + 1] * f
        return m
    return torch.einsum("bc,bch->bh", g, torch.stack(outputs, dim=1))


def ple(x, levels, towers=None, clipped=None, ordered=False, *, task_gates_read_shared=()):
    """x [B, width]; levels[j] = (specific: K lists of ms experts, shared: mc experts, gates: K (W, b),
    shared_gate: (W, b) or None at the last level), an expert a list of (W, b); towers: K (hidden [(W, b)…],
    (w_out [1, ·], b_out)) or None.  Returns (per level (representations [B, K + 1, H] — [B, K, H] at the last
    level —, task gates [B, K, ms + mc], shared gate [B, K ms + mc] or None), logits [B, K], probs [B, K]);
    logits and probs are None without towers.  `clipped` collects every ReLU's share of negative
    pre-activations; ordered: every sum in a fixed order (mmoe_ref.linear).
    task_gates_read_shared: levels at which the task gates (wrongly) read x_s — what a kernel that mixed up its
    inputs would compute; tests/test_ple_ref.py uses it to show that the cases would notice."""
    K = len(levels[0][2])
    xk, xs = [x] * K, x
    out = []
    for j, (specific, shared, gates, shared_gate) in enumerate(levels):
        fk = [[stack(xk[k], layers, clipped, ordered) for layers in specific[k]] for k in range(K)]
        fs = [stack(xs, layers, clipped, ordered) for layers in shared]
        gk = [gate(xs if j in task_gates_read_shared else xk[k], gates[k], ordered) for k in range(K)]
        if not ordered and not any(fk):  # no task experts: MMoE's mix, in mmoe_ref's very operation (the same bits)
            new = list(torch.einsum("bke,beh->bkh", torch.stack(gk, dim=1), torch.stack(fs, dim=1)).unbind(dim=1))
        else:
            new = [mix(gk[k], fk[k] + fs, ordered) for k in range(K)]
        gs = None
        if shared_gate is not None:
            gs = gate(xs, shared_gate, ordered)
            xs = mix(gs, [f for task in fk for f in task] + fs, ordered)
            out.append((torch.stack(new + [xs], dim=1), torch.stack(gk, dim=1), gs))
        else:
            out.append((torch.stack(new, dim=1), torch.stack(gk, dim=1), None))
        xk = new
    if towers is None:
        return out, None, None
    logits = []
    for k, (hidden, (w_out, b_out)) in enumerate(towers):
        t = stack(xk[k], hidden, clipped, ordered)
        logits.append(linear(t, w_out.reshape(1, -1), b_out.reshape(1, 1), ordered))
    logits = torch.cat(logits, dim=1)
    return out, logits, torch.sigmoid(logits)


def _linears(p, prefix):
    """[(W, b)…] of the Sequential at `prefix` (its Linear modules in index order)."""
    idx = sorted({int(k[len(prefix):].split(".")[0]) for k in p if k.startswith(prefix) and k.endswith(".weight")})
    return [(p[f"{prefix}{i}.weight"], p[f"{prefix}{i}.bias"]) for i in idx]


def _count(p, prefix):
    return len({k[len(prefix):].split(".")[0] for k in p if k.startswith(prefix)})


def model_parts(p):
    """(levels, towers) of a rankops.PLE state_dict, in ple()'s form."""
    L = _count(p, "levels.")
    K = _count(p, "tower_outputs.")
    levels = []
    for j in range(L):
        pre = f"levels.{j}."
        ms = _count(p, pre + "specific_experts.0.")
        mc = _count(p, pre + "shared_experts.")
        specific = [[_linears(p, f"{pre}specific_experts.{k}.{i}.") for i in range(ms)] for k in range(K)]
        shared = [_linears(p, f"{pre}shared_experts.{i}.") for i in range(mc)]
        gates = [(p[f"{pre}gates.{k}.weight"], p[f"{pre}gates.{k}.bias"]) for k in range(K)]
        sg = (p[pre + "shared_gate.weight"], p[pre + "shared_gate.bias"]) if pre + "shared_gate.weight" in p else None
        levels.append((specific, shared, gates, sg))
    towers = [(_linears(p, f"towers.{k}."), (p[f"tower_outputs.{k}.weight"], p[f"tower_outputs.{k}.bias"]))
              for k in range(K)]
    return levels, towers


def forward(p, dense, category, keep=None, ordered=False):
    """(probabilities [B, K], logits [B, K]) of a rankops.PLE state_dict, in p's dtype.  keep: as
    mmoe_ref.model_row (fields zeroed where an id is out of range)."""
    x = model_row(p, dense, category, keep)
    levels, towers = model_parts(p)
    _, logits, probs = ple(x, levels, towers, ordered=ordered)
    return probs, logits


# ---------------------------------------------------------------- seeded inputs of the GPU tests

# Seeds chosen so that every case sits inside the bands of tests/test_ple_ref.py (every ReLU clips 0.2-0.8 of
# its inputs, the mean largest gate lies between 1.5 / columns and 0.85 with at most 0.15 of rows above 0.95 —
# two-column gates leave 0.75-0.85 —, and the three shared-path perturbations move the logits)
CASE_SEEDS = {"tile_edge": 2044, "odd": 2029, "one_task": 2027}


def _scaled_stack(g, k, units):
    layers = []
    for n in units:
        layers.append(_linear(g, n, k, WEIGHT_SCALE))
        k = n
    return layers, k


def op_inputs(c, seed=None):
    """float32 CPU inputs of one op-level case: the row buffer [B, width + ROW_PAD] (x = its first `width`
    columns), levels and towers in ple()'s form."""
    name, width, L, K, ms, mc, eu, tu, B = c
    seed = CASE_SEEDS.get(name, 2025) if seed is None else seed
    g = torch.Generator().manual_seed(seed + 131 * width + 17 * (K * ms + mc) + 7 * K + B + len(eu) + 3 * len(tu) + 1009 * L)
    rows = torch.randn(B, width + ROW_PAD, generator=g) * X_STD
    levels, H = [], eu[-1]
    for j in range(L):
        k_in = width if j == 0 else H
        scale = EXTREME_GATE_SCALE if name == EXTREME else GATE_SCALE if j == 0 else DEEP_GATE_SCALE
        specific = [[_scaled_stack(g, k_in, eu)[0] for _ in range(ms)] for _ in range(K)]
        shared = [_scaled_stack(g, k_in, eu)[0] for _ in range(mc)]
        gates = [_linear(g, ms + mc, k_in, scale) for _ in range(K)]
        shared_gate = _linear(g, K * ms + mc, k_in, scale) if j < L - 1 else None
        levels.append((specific, shared, gates, shared_gate))
    towers = []
    for _ in range(K):
        hidden, last = _scaled_stack(g, H, tu)
        w, b = _linear(g, 1, last)
        towers.append((hidden, (w, b)))
    return rows, levels, towers


_REFS = {}


def op_reference(c, dtype=torch.float64, clipped=None, ordered=False):
    """(levels, logits, probs) of one op-level case from the restatement in `dtype`; the float64 result is
    computed once and shared (do not modify it)."""
    key = (c[0], dtype, ordered)
    if clipped is None and key in _REFS:
        return _REFS[key]
    rows, levels, towers = op_inputs(c)
    out = ple(rows[:, :c[1]].to(dtype), cast(levels, dtype), cast(towers, dtype), clipped, ordered)
    if clipped is None:
        _REFS[key] = out
    return out


def flat(out):
    """(representations, gates, logits, probs) of ple()'s result as four lists of tensors: what the four
    tolerances bound."""
    levels, logits, probs = out
    reps = [lv[0] for lv in levels]
    gates = [g for lv in levels for g in lv[1:] if g is not None]
    return reps, gates, [logits] if logits is not None else [], [probs] if probs is not None else []


def build_model(mc, seed=42):
    """Seeded rankops.PLE (CPU, eval) of a model case, its gate weights and biases x GATE_SCALE (level 0) or
    DEEP_GATE_SCALE (later levels)."""
    import rankops
    _, which, _, kw = mc
    torch.manual_seed(seed)
    model = rankops.PLE(None, vocab_sizes=vocab(which), **kw)
    with torch.no_grad():
        for j, level in enumerate(model.levels):
            for gate_ in level.all_gates():
                gate_.weight.mul_(GATE_SCALE if j == 0 else DEEP_GATE_SCALE)
                gate_.bias.mul_(GATE_SCALE if j == 0 else DEEP_GATE_SCALE)
    return model.eval()


def model_inputs(mc, seed=1000):
    import helpers as H
    _, which, B, _ = mc
    return H.dcn_inputs(B, vocab(which), seed)
