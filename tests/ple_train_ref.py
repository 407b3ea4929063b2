"""Training restatement of PLE: tests/ple_ref.py's definition with an explicit dropout keep-multiplier per
site (None in eval), differentiated by torch autograd in the dtype of its inputs (the tests run it in
float64), plus the loss, the seeded inputs and the gradient tolerances of tests/test_gpu_ple_train.py.  The
stack with its keep-multipliers, the leaves / flat helpers and the loss coefficients are
tests/mmoe_train_ref.py's.

Dropout.  A site is one ReLU's output.  With NE = K ms + mc stacks per level (task k's i-th at k ms + i, the
shared i-th at K ms + i), De expert layers and Dt tower layers: expert s of level j, layer l is site
(j NE + s) De + l, tower k layer l is site L NE De + k Dt + l.  `keeps[site]` is a [B, n] tensor holding 0
where the element is dropped and 1 / (1 - p) where it is kept.  `keeps=None` is eval: the formula is then
ple_ref's, operation for operation, and the results are equal bit for bit (tests/test_ple_train_ref.py).

Loss.  A fixed random linear functional of the outputs (mmoe_train_ref.loss_coeffs, N(0, 1) coefficients):
with towers sum(c_l logits) + sum(c_p probs), without towers sum(c_m reps) over the last level's
representations; `use` selects the terms (the "cannot hide" checks of the CPU test use all three).

Tolerances.  A tolerance t is used as |got - ref| <= t * (1 + |ref|) against the float64 gradients.  Each is
50 x the drift of this same restatement differentiated in float32 with fixed-order forward sums
(`ordered=True`) against float64, drift = max |f32 - f64| / (1 + |f64|) over the seeded inputs of the GPU
tests: every ordinary case of GRAD_CASES, with towers and without, and the model-level cases (dropout 0.1,
masks from a seeded CPU generator).  50 x is what every other kernel of this family gets over the same kind
of drift.  Gradients are grouped by what they multiply: dx (the input rows; at model level the embedding
tables), dw (every expert, tower and head weight and bias) and dgate (the gates' weights and biases).
`extreme_gate` has its own three.  tests/test_ple_train_ref.py measures the drifts again and fails if a
constant lies outside 25-100 x of what it measures.  Nothing is tuned against a GPU result.  Measured
(torch 2.x, CPU):

    ordinary   dx    drift 1.91e-06  ->  DX_TOL    9.5e-05
               dw    drift 6.08e-06  ->  DW_TOL    3.0e-04
               dgate drift 6.10e-06  ->  DGATE_TOL 3.0e-04
    extreme    dx    drift 3.62e-05  ->  EXTREME_DX_TOL    1.8e-03
               dw    drift 4.99e-05  ->  EXTREME_DW_TOL    2.5e-03
               dgate drift 1.37e-05  ->  EXTREME_DGATE_TOL 6.8e-04
"""
from __future__ import annotations

import torch

import mmoe_train_ref as M
import ple_ref as R
from mmoe_train_ref import cpu_keeps, flat, leaves, loss_coeffs  # noqa: F401

DX_TOL = 9.5e-05
DW_TOL = 3.0e-04
DGATE_TOL = 3.0e-04
EXTREME_DX_TOL = 1.8e-03
EXTREME_DW_TOL = 2.5e-03
EXTREME_DGATE_TOL = 6.8e-04

# NE = 18 stacks: the grouped calls are chunked (16 + 2); 200 rows give the weight-gradient reduction four
# 64-row slabs (mmoe_train_ref.SLAB_CASE)
MANY_CASE = ("many", 20, 2, 3, 5, 3, (12, 8), (8,), 200)
GRAD_CASES = list(R.OP_CASES) + [MANY_CASE]
CASE_SEEDS = {}  # a seed other than ple_ref's for a case of this file (none needed: see test_ple_train_ref.py)
DROPOUT_P = 0.1

# model-level cases: (name, batch, constructor arguments), small vocabulary
MODEL_CASES = [("default_300", 300, {}), ("default_17", 17, {}), ("alt_300", 300, R.ALT_CONFIG), ("alt_17", 17, R.ALT_CONFIG)]


def case(name):
    return next(c for c in GRAD_CASES if c[0] == name)


def tolerances(name):
    """(dx, dw, dgate) tolerances of a case."""
    if name == R.EXTREME:
        return EXTREME_DX_TOL, EXTREME_DW_TOL, EXTREME_DGATE_TOL
    return DX_TOL, DW_TOL, DGATE_TOL


# ---------------------------------------------------------------- the definition

WRONG = ("shared_detached", "task_stacks_miss_shared", "last_shared_to_task0")


def ple(x, levels, towers=None, keeps=None, clipped=None, ordered=False, wrong=None):
    """ple_ref.ple with dropout multipliers: keeps = {site: [B, n] tensor} or None (eval).  `wrong` names a
    backward path that is deliberately broken (the forward values are unchanged): the shared representation
    detached between levels, the task stacks missing the shared mixture's gradient, or the last level's
    shared stacks taking task 0's gradient only — what a backward that lost one of PLE's own paths would
    compute; tests/test_ple_train_ref.py uses them to show that the cases would notice."""
    K, L = len(levels[0][2]), len(levels)
    ms, mc, De = len(levels[0][0][0]) if levels[0][0] else 0, len(levels[0][1]), len(levels[0][1][0])
    NE = K * ms + mc
    xk, xs = [x] * K, x
    out = []
    for j, (specific, shared, gates, shared_gate) in enumerate(levels):
        site = lambda s: (j * NE + s) * De  # noqa: E731
        fk = [[M.stack(xk[k], layers, keeps, site(k * ms + i), clipped, ordered) for i, layers in enumerate(specific[k])]
              for k in range(K)]
        fs = [M.stack(xs, layers, keeps, site(K * ms + i), clipped, ordered) for i, layers in enumerate(shared)]
        gk = [R.gate(xk[k], gates[k], ordered) for k in range(K)]
        if not ordered and not any(fk) and wrong is None:  # ple_ref's very operation (the same bits)
            new = list(torch.einsum("bke,beh->bkh", torch.stack(gk, dim=1), torch.stack(fs, dim=1)).unbind(dim=1))
        else:
            new = []
            for k in range(K):
                own = fs
                if wrong == "last_shared_to_task0" and j == L - 1 and k > 0:
                    own = [f.detach() for f in fs]
                new.append(R.mix(gk[k], fk[k] + own, ordered))
        if shared_gate is not None:
            gs = R.gate(xs, shared_gate, ordered)
            tasks = [f for task in fk for f in task]
            if wrong == "task_stacks_miss_shared":
                tasks = [f.detach() for f in tasks]
            xs = R.mix(gs, tasks + fs, ordered)
            out.append((torch.stack(new + [xs], dim=1), torch.stack(gk, dim=1), gs))
            if wrong == "shared_detached":
                xs = xs.detach()
        else:
            out.append((torch.stack(new, dim=1), torch.stack(gk, dim=1), None))
        xk = new
    if towers is None:
        return out, None, None
    Dt = len(towers[0][0])
    logits = []
    for k, (hidden, (w_out, b_out)) in enumerate(towers):
        t = M.stack(xk[k], hidden, keeps, L * NE * De + k * Dt, clipped, ordered)
        logits.append(R.linear(t, w_out.reshape(1, -1), b_out.reshape(1, 1), ordered))
    logits = torch.cat(logits, dim=1)
    return out, logits, torch.sigmoid(logits)


def forward(p, dense, category, keeps=None, ordered=False):
    """(probabilities, logits) of a rankops.PLE state_dict in p's dtype, dropout multipliers as in ple."""
    x = R.model_row(p, dense, category)
    levels, towers = R.model_parts(p)
    _, logits, probs = ple(x, levels, towers, keeps, ordered=ordered)
    return probs, logits


def sites_of(L, K, ms, mc, eu, tu):
    """[(site, n)…] of a configuration."""
    NE, De, Dt = K * ms + mc, len(eu), len(tu)
    return ([((j * NE + s) * De + l, eu[l]) for j in range(L) for s in range(NE) for l in range(De)]
            + [(L * NE * De + k * Dt + l, tu[l]) for k in range(K) for l in range(Dt)])


# ---------------------------------------------------------------- losses and gradients

def split_levels(levels):
    """(stack tensors, gate tensors) of levels in ple()'s form, each flattened level by level: the stacks
    task-major then the shared, the K gates then the shared gate; a None bias has no entry."""
    stacks, gates = [], []
    for specific, shared, gs, shared_gate in levels:
        stacks += flat(specific) + flat(shared)
        gates += flat(gs) + flat(shared_gate)
    return stacks, gates


def op_gradients(x, levels, towers, dtype=torch.float64, keeps=None, ordered=False, use=("logits", "probs"), wrong=None):
    """Outputs and gradients of the op-level loss: {"out": ple()'s result, "dx": …, "experts": [dW, db…] (every
    level's stacks), "gates": […], "towers": […] (hidden layers then the output layer, tower-major)}.  use:
    the terms of the loss, of "reps" (the last level's representations), "logits", "probs"."""
    x = leaves(x, dtype)
    levels, towers = leaves(levels, dtype), leaves(towers, dtype)
    keeps = None if keeps is None else {s: k.to(dtype) for s, k in keeps.items()}
    out = ple(x, levels, towers, keeps, ordered=ordered, wrong=wrong)
    reps = out[0][-1][0]
    B, K, H = reps.shape
    cm, cl, cp = (c.to(dtype) for c in loss_coeffs(B, K, H))
    loss = torch.zeros((), dtype=dtype)
    if "reps" in use:
        loss = loss + (cm * reps).sum()
    if towers is not None and "logits" in use:
        loss = loss + (cl * out[1]).sum()
    if towers is not None and "probs" in use:
        loss = loss + (cp * out[2]).sum()
    loss.backward()
    zero = lambda ts: [t.grad if t.grad is not None else torch.zeros_like(t) for t in ts]  # noqa: E731
    stacks, gates = split_levels(levels)
    detached = ([tuple(None if t is None else t.detach() for t in lv) for lv in out[0]],
                None if out[1] is None else out[1].detach(), None if out[2] is None else out[2].detach())
    return dict(out=detached, dx=zero([x])[0], experts=zero(stacks), gates=zero(gates), towers=zero(flat(towers)))


def model_gradients(p, dense, category, dtype=torch.float64, keeps=None, ordered=False):
    """(probs, logits, {state_dict key: gradient}) of the model-level loss sum(c_l logits) + sum(c_p probs)."""
    q = {k: (v.detach().to(dtype).clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in p.items()}
    keeps = None if keeps is None else {s: k.to(dtype) for s, k in keeps.items()}
    probs, logits = forward(q, dense, category, keeps, ordered)
    B, K = logits.shape
    _, cl, cp = (c.to(dtype) for c in loss_coeffs(B, K, 1))
    ((cl * logits).sum() + (cp * probs).sum()).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in q.items() if v.is_floating_point()}
    return probs.detach(), logits.detach(), grads


def group_of(key):
    """The tolerance group (0 dx, 1 dw, 2 dgate) of a state_dict key."""
    return 0 if key.startswith("embeddings.") else 2 if ".gates." in key or ".shared_gate." in key else 1


def op_inputs(c):
    """ple_ref.op_inputs, also for the cases that are only in GRAD_CASES."""
    return R.op_inputs(c, CASE_SEEDS.get(c[0]))


_REFS = {}


def op_reference(c, towers=True):
    """float64 outputs and gradients of one op-level case, computed once: with towers the loss over logits and
    probs, without towers over the last level's representations."""
    key = (c[0], towers)
    if key not in _REFS:
        rows, levels, tw = op_inputs(c)
        _REFS[key] = op_gradients(rows[:, :c[1]], levels, tw if towers else None, use=("logits", "probs") if towers else ("reps",))
    return _REFS[key]


def build_model(kw, seed=42, **flags):
    """Seeded rankops.PLE on the small vocabulary (CPU), its gates scaled as ple_ref.build_model's."""
    import helpers as Hh
    import rankops
    torch.manual_seed(seed)
    model = rankops.PLE(None, vocab_sizes=Hh.SMALL_VOCAB, **kw, **flags)
    with torch.no_grad():
        for j, level in enumerate(model.levels):
            for gate_ in level.all_gates():
                gate_.weight.mul_(R.GATE_SCALE if j == 0 else R.DEEP_GATE_SCALE)
                gate_.bias.mul_(R.GATE_SCALE if j == 0 else R.DEEP_GATE_SCALE)
    return model


def model_inputs(B, seed=1000):
    """(dense [B, 16], category {field: [B]}) on the small vocabulary."""
    return M.model_inputs(B, seed)


def model_sites(model):
    return sites_of(model.num_levels, len(model.task_names), model.num_specific_experts, model.num_shared_experts,
                    model.expert_hidden_units, model.tower_hidden_units)


def drifts():
    """{"ordinary": [dx, dw, dgate], "extreme": […]}: float32 (ordered) against float64 gradient drift."""
    out = {"ordinary": [0.0, 0.0, 0.0], "extreme": [0.0, 0.0, 0.0]}

    def upd(which, i, a, b):
        out[which][i] = max(out[which][i], R.rel_err(a, b))
    for c in GRAD_CASES:
        rows, levels, towers = op_inputs(c)
        which = "extreme" if c[0] == R.EXTREME else "ordinary"
        for tw in (True, False):
            ref = op_reference(c, tw)
            got = op_gradients(rows[:, :c[1]], levels, towers if tw else None, torch.float32, ordered=True,
                               use=("logits", "probs") if tw else ("reps",))
            upd(which, 0, got["dx"], ref["dx"])
            for a, b in zip(got["experts"] + got["towers"], ref["experts"] + ref["towers"]):
                upd(which, 1, a, b)
            for a, b in zip(got["gates"], ref["gates"]):
                upd(which, 2, a, b)
    for name, B, kw in MODEL_CASES:
        model = build_model(kw)
        p = model.state_dict()
        dense, cat = model_inputs(B)
        keeps = cpu_keeps(model_sites(model), B, DROPOUT_P)
        _, _, ref = model_gradients(p, dense, cat, keeps=keeps)
        _, _, got = model_gradients(p, dense, cat, torch.float32, keeps=keeps, ordered=True)
        for k in ref:
            upd("ordinary", group_of(k), got[k], ref[k])
    return out


if __name__ == "__main__":
    for which, d in drifts().items():
        for n, v in zip(("dx", "dw", "dgate"), d):
            print(f"{which:9s} {n:6s} drift {v:.2e}  ->  {50 * v:.1e}")
