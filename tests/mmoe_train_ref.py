"""Training restatement of MMoE: tests/mmoe_ref.py's definition with an explicit dropout keep-multiplier
per site (None in eval), differentiated by torch autograd in the dtype of its inputs (the tests run it
in float64), plus the loss, the seeded inputs and the gradient tolerances of tests/test_gpu_mmoe_train.py.

Dropout.  A site is one ReLU's output: expert e layer l is site e * De + l, tower k layer l is site
E * De + k * Dt + l (De, Dt = the numbers of expert and tower layers).  `keeps[site]` is a [B, n] tensor
holding 0 where the element is dropped and 1 / (1 - p) where it is kept; the layer's output is
relu(z) * keeps[site].  `keeps=None` (or a missing site) is eval: the formula is then mmoe_ref's, operation
for operation, and the results are equal bit for bit (tests/test_mmoe_train_ref.py).

Loss.  The op-level tests differentiate a fixed random linear functional of the outputs,
loss = sum(c_m * mixed) + sum(c_l * logits) + sum(c_p * probs) (`loss_coeffs`, N(0, 1) coefficients), so
that every output's backward is exercised with gradients of ordinary size.  The model-level tests use
the same functional of (logits, probs).

Tolerances.  A tolerance t is used as |got - ref| <= t * (1 + |ref|) against the float64 gradients.  Each
is 50 x the drift of this same restatement differentiated in float32 against float64, drift = max |f32 -
f64| / (1 + |f64|) over the seeded inputs of the GPU tests: every ordinary op-level case of GRAD_CASES and
the model-level cases (with dropout 0.1, masks drawn from a seeded CPU generator: the engine's masks differ
in which elements they keep, not in how many).  The float32 run takes every forward sum in a fixed
order (`ordered=True`), for the reason mmoe_ref.py gives.  Gradients are grouped by what they multiply:
dx (the input rows; at model level the embedding tables), dw (every expert, tower and head weight and
bias) and dgate (the gates' weights and biases).  `extreme_gate` (near-one-hot gates) has its own
constants.  tests/test_mmoe_train_ref.py measures the drifts again and fails if a constant lies outside
25-100 x of what it measures.  Measured (torch 2.x, CPU):

    ordinary   dx    drift 9.92e-07  ->  DX_TOL    5.0e-05
               dw    drift 2.30e-06  ->  DW_TOL    1.1e-04
               dgate drift 2.02e-06  ->  DGATE_TOL 1.0e-04
    extreme    dx    drift 2.71e-05  ->  EXTREME_DX_TOL    1.4e-03
               dw    drift 3.37e-06  ->  EXTREME_DW_TOL    1.7e-04
               dgate drift 8.88e-07  ->  EXTREME_DGATE_TOL 4.4e-05
"""
from __future__ import annotations

import torch

import mmoe_ref as R

DX_TOL = 5.0e-05
DW_TOL = 1.1e-04
DGATE_TOL = 1.0e-04
EXTREME_DX_TOL = 1.4e-03
EXTREME_DW_TOL = 1.7e-04
EXTREME_DGATE_TOL = 4.4e-05

# rk_gemm_wgrad's kernel reduces 64 rows per step (kWgR) and gives a workgroup a slab of at least one
# step, one slab per CU at most: a batch of 200 rows makes 4 slabs (64 + 64 + 64 + 8 rows) while the widths
# stay small, so the fixed-order reduction over slabs has more than one term and a ragged last step.
SLAB_CASE = ("slabs", 20, 3, 2, (12, 8), (8,), 200)
GRAD_CASES = [R.case(n) for n in ("one_row", "tile_edge", "odd", "deep", "one_expert", "wide", "extreme_gate")] + [SLAB_CASE]
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

def stack(x, layers, keeps, site0, clipped=None, ordered=False):
    """Linear + ReLU (+ dropout multiplier keeps[site0 + l]) per (W, b)."""
    for l, (W, b) in enumerate(layers):
        z = R.linear(x, W, b, ordered)
        if clipped is not None:
            clipped.append(float((z < 0).double().mean()))
        x = torch.relu(z)
        k = None if keeps is None else keeps.get(site0 + l)
        if k is not None:
            x = x * k
    return x


def mmoe(x, experts, gates, towers=None, keeps=None, clipped=None, ordered=False):
    """mmoe_ref.mmoe with dropout multipliers: keeps = {site: [B, n] tensor} or None (eval)."""
    E, De = len(experts), len(experts[0])
    f = torch.stack([stack(x, layers, keeps, e * De, clipped, ordered) for e, layers in enumerate(experts)], dim=1)
    if ordered:
        g = []
        for W, b in gates:
            z = R.linear(x, W, b, True)
            ex = torch.exp(z - z.max(dim=1, keepdim=True).values)
            total = torch.zeros(x.shape[0], 1, dtype=x.dtype)
            for e in range(ex.shape[1]):
                total = total + ex[:, e:e + 1]
            g.append(ex / total)
        g = torch.stack(g, dim=1)
        m = torch.zeros(x.shape[0], g.shape[1], f.shape[2], dtype=x.dtype)
        for e in range(f.shape[1]):
            m = m + g[:, :, e:e + 1] * f[:, e:e + 1, :]
    else:
        g = torch.stack([torch.softmax(R.linear(x, W, b), dim=1) for W, b in gates], dim=1)
        m = torch.einsum("bke,beh->bkh", g, f)
    if towers is None:
        return m, g
    Dt = len(towers[0][0])
    logits = []
    for k, (hidden, (w_out, b_out)) in enumerate(towers):
        t = stack(m[:, k], hidden, keeps, E * De + k * Dt, clipped, ordered)
        logits.append(R.linear(t, w_out.reshape(1, -1), b_out.reshape(1, 1), ordered))
    logits = torch.cat(logits, dim=1)
    return m, g, logits, torch.sigmoid(logits)


def forward(p, dense, category, keeps=None, ordered=False):
    """(probabilities, logits) of a rankops.MMoE state_dict in p's dtype, dropout multipliers as in mmoe."""
    x = R.model_row(p, dense, category)
    experts, gates, towers = R.model_parts(p)
    _, _, logits, probs = mmoe(x, experts, gates, towers, keeps, ordered=ordered)
    return probs, logits


# ---------------------------------------------------------------- losses and gradients

def loss_coeffs(B, K, H, seed=77):
    g = torch.Generator().manual_seed(seed + 1000 * B + 10 * K + H)
    return (torch.randn(B, K, H, generator=g, dtype=torch.float64), torch.randn(B, K, generator=g, dtype=torch.float64),
            torch.randn(B, K, generator=g, dtype=torch.float64))


def leaves(obj, dtype):
    """A copy of nested (W, b) lists as autograd leaves in dtype (None stays None)."""
    if obj is None:
        return None
    if isinstance(obj, torch.Tensor):
        return obj.detach().to(dtype).clone().requires_grad_(True)
    return type(obj)(leaves(o, dtype) for o in obj)


def flat(obj):
    if obj is None:
        return []
    if isinstance(obj, torch.Tensor):
        return [obj]
    return [t for o in obj for t in flat(o)]


def op_gradients(x, experts, gates, towers, dtype=torch.float64, keeps=None, ordered=False,
                 use=("mixed", "logits", "probs")):
    """Outputs and gradients of the op-level loss: {"out": (mixed, gate_probs[, logits, probs]), "dx": …,
    "experts": [(dW, db)…] flattened expert-major, "gates": […], "towers": […] (hidden layers then the output
    layer, tower-major)}; a None bias has no entry."""
    x = leaves(x, dtype)
    experts, gates, towers = leaves(experts, dtype), leaves(gates, dtype), leaves(towers, dtype)
    keeps = None if keeps is None else {s: k.to(dtype) for s, k in keeps.items()}
    out = mmoe(x, experts, gates, towers, keeps, ordered=ordered)
    B, K, H = out[0].shape
    cm, cl, cp = (c.to(dtype) for c in loss_coeffs(B, K, H))
    loss = torch.zeros((), dtype=dtype)
    if "mixed" in use:
        loss = loss + (cm * out[0]).sum()
    if towers is not None and "logits" in use:
        loss = loss + (cl * out[2]).sum()
    if towers is not None and "probs" in use:
        loss = loss + (cp * out[3]).sum()
    loss.backward()
    zero = lambda ts: [t.grad if t.grad is not None else torch.zeros_like(t) for t in ts]
    return dict(out=tuple(o.detach() for o in out), dx=zero([x])[0], experts=zero(flat(experts)), gates=zero(flat(gates)),
                towers=zero(flat(towers)))


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
    return 0 if key.startswith("embeddings.") else 2 if key.startswith("gates.") else 1


def cpu_keeps(sites, B, p, seed=5):
    """Seeded Bernoulli keep-multipliers {site: [B, n]} for sites = [(site, n)…] (float64)."""
    g = torch.Generator().manual_seed(seed)
    return {s: (torch.rand(B, n, generator=g, dtype=torch.float64) >= p).double() / (1 - p) for s, n in sites}


def sites_of(E, K, eu, tu):
    """[(site, n)…] of a configuration."""
    De, Dt = len(eu), len(tu)
    return ([(e * De + l, eu[l]) for e in range(E) for l in range(De)]
            + [(E * De + k * Dt + l, tu[l]) for k in range(K) for l in range(Dt)])


def op_inputs(c):
    """mmoe_ref.op_inputs, also for the cases that are only in GRAD_CASES."""
    return R.op_inputs(c)


_REFS = {}


def op_reference(c):
    """float64 outputs and gradients of one op-level case (all three outputs in the loss), computed once."""
    if c[0] not in _REFS:
        rows, experts, gates, towers = op_inputs(c)
        _REFS[c[0]] = op_gradients(rows[:, :c[1]], experts, gates, towers)
    return _REFS[c[0]]


def build_model(kw, seed=42, **flags):
    """Seeded rankops.MMoE on the small vocabulary (CPU), its gates scaled as mmoe_ref.build_model's."""
    import helpers as Hh
    import rankops
    torch.manual_seed(seed)
    model = rankops.MMoE(None, vocab_sizes=Hh.SMALL_VOCAB, **kw, **flags)
    with torch.no_grad():
        for gate in model.gates:
            gate.weight.mul_(R.GATE_SCALE)
            gate.bias.mul_(R.GATE_SCALE)
    return model


def model_inputs(B, seed=1000):
    """(dense [B, 16], category {field: [B]}) on the small vocabulary."""
    import helpers as Hh
    inp = Hh.dcn_inputs(B, Hh.SMALL_VOCAB, seed)
    return inp["dense"], inp["category"]


def drifts():
    """{"ordinary": [dx, dw, dgate], "extreme": […]}: float32 (ordered) against float64 gradient drift."""
    out = {"ordinary": [0.0, 0.0, 0.0], "extreme": [0.0, 0.0, 0.0]}

    def upd(which, i, a, b):
        out[which][i] = max(out[which][i], R.rel_err(a, b))
    for c in GRAD_CASES:
        rows, experts, gates, towers = op_inputs(c)
        ref = op_reference(c)
        got = op_gradients(rows[:, :c[1]], experts, gates, towers, torch.float32, ordered=True)
        which = "extreme" if c[0] == R.EXTREME else "ordinary"
        upd(which, 0, got["dx"], ref["dx"])
        for a, b in zip(got["experts"] + got["towers"], ref["experts"] + ref["towers"]):
            upd(which, 1, a, b)
        for a, b in zip(got["gates"], ref["gates"]):
            upd(which, 2, a, b)
    for name, B, kw in MODEL_CASES:
        model = build_model(kw)
        p = model.state_dict()
        dense, cat = model_inputs(B)
        keeps = cpu_keeps(sites_of(model.num_experts, len(model.task_names), model.expert_hidden_units,
                                   model.tower_hidden_units), B, DROPOUT_P)
        _, _, ref = model_gradients(p, dense, cat, keeps=keeps)
        _, _, got = model_gradients(p, dense, cat, torch.float32, keeps=keeps, ordered=True)
        for k in ref:
            upd("ordinary", group_of(k), got[k], ref[k])
    return out


if __name__ == "__main__":
    for which, d in drifts().items():
        for n, v in zip(("dx", "dw", "dgate"), d):
            print(f"{which:9s} {n:6s} drift {v:.2e}  ->  {50 * v:.1e}")
