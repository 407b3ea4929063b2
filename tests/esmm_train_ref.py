"""Training restatement of ESMM: tests/esmm_ref.py's definition with an explicit dropout keep-multiplier
per site (None in eval), differentiated by torch autograd in the dtype of its inputs (the tests run it
in float64), plus the losses, the seeded inputs and the gradient tolerances of
tests/test_gpu_esmm_train.py.

Dropout.  A site is one ReLU's output: tower k layer l is site k * Dt + l (Dt = the number of tower
layers).  `keeps[site]` is a [B, n] tensor holding 0 where the element is dropped and 1 / (1 - p) where it
is kept; the layer's output is relu(z) * keeps[site].  `keeps=None` (or a missing site) is eval: the
formula is then esmm_ref's, operation for operation, and the results are equal bit for bit
(tests/test_esmm_train_ref.py).

Loss.  The op-level tests differentiate a fixed random linear functional of the outputs,
loss = sum(c_p * probs) + sum(c_l * logits) + sum(c_c * cond) (mmoe_train_ref.loss_coeffs' generator,
N(0, 1) coefficients), so that every output's backward is exercised with gradients of ordinary size.  The
model-level tests use the same functional of (probs, logits).

Tolerances.  A tolerance t is used as |got - ref| <= t * (1 + |ref|) against the float64 gradients.  Each
is 50 x the drift of this same restatement differentiated in float32 (`ordered=True`) against float64
over the seeded inputs of the GPU tests: every op-level case of GRAD_CASES and the model-level cases (with
dropout 0.1, masks drawn from a seeded CPU generator: the engine's masks differ in which elements they
keep, not in how many).  Gradients are grouped by what they multiply: dx (the input rows; at model level
the embedding tables) and dw (every tower and head weight and bias).  The gradient of
rk_esmm_joint_backward's fold (JOINT_TOL) is measured the same way on the logits of the loss cases of
esmm_ref.  tests/test_esmm_train_ref.py measures the drifts again and fails if a constant lies outside
25-100 x of what it measures.  Measured (torch 2.x, CPU):

    dx    drift 2.87e-06  ->  DX_TOL    1.4e-04
    dw    drift 4.96e-06  ->  DW_TOL    2.5e-04
    joint drift 3.02e-07  ->  JOINT_TOL 1.5e-05
"""
from __future__ import annotations

import torch

import esmm_ref as R
import mmoe_ref as M
from mmoe_train_ref import cpu_keeps, flat, leaves  # noqa: F401

DX_TOL = 1.4e-04
DW_TOL = 2.5e-04
JOINT_TOL = 1.5e-05

# 200 rows make rk_gemm_wgrad's reduction four slabs with a ragged last step (mmoe_train_ref.SLAB_CASE)
SLAB_CASE = ("slabs", 20, 3, (12, 8), 200)
GRAD_CASES = list(R.OP_CASES) + [SLAB_CASE]
DROPOUT_P = 0.1

# model-level cases: (name, batch, constructor arguments), small vocabulary
MODEL_CASES = [("default_300", 300, {}), ("default_17", 17, {}), ("alt_300", 300, R.ALT_CONFIG),
               ("alt_17", 17, R.ALT_CONFIG)]


# ---------------------------------------------------------------- the definition

def stack(x, layers, keeps, site0, ordered=False):
    """Linear + ReLU (+ dropout multiplier keeps[site0 + l]) per (W, b)."""
    for l, (W, b) in enumerate(layers):
        x = torch.relu(M.linear(x, W, b, ordered))
        k = None if keeps is None else keeps.get(site0 + l)
        if k is not None:
            x = x * k
    return x


def esmm(x, towers, keeps=None, ordered=False):
    """esmm_ref.esmm with dropout multipliers: keeps = {site: [B, n] tensor} or None (eval)."""
    Dt = len(towers[0][0])
    logits = []
    for k, (hidden, (w_out, b_out)) in enumerate(towers):
        t = stack(x, hidden, keeps, k * Dt, ordered)
        logits.append(M.linear(t, w_out.reshape(1, -1), None if b_out is None else b_out.reshape(1, 1), ordered))
    logits = torch.cat(logits, dim=1)
    probs, cond = R.chain(logits)
    return probs, logits, cond


def forward(p, dense, category, keeps=None, ordered=False):
    """(probabilities, logits) of a rankops.ESMM state_dict in p's dtype, dropout multipliers as in esmm."""
    probs, logits, _ = esmm(R.model_row(p, dense, category), R.model_parts(p), keeps, ordered)
    return probs, logits


# ---------------------------------------------------------------- losses and gradients

def loss_coeffs(B, K, seed=77):
    """(c_p, c_l, c_c), each [B, K] float64."""
    g = torch.Generator().manual_seed(seed + 1000 * B + 10 * K)
    return tuple(torch.randn(B, K, generator=g, dtype=torch.float64) for _ in range(3))


def op_gradients(x, towers, dtype=torch.float64, keeps=None, ordered=False, use=("probs", "logits", "cond")):
    """Outputs and gradients of the op-level loss: {"out": (probs, logits, cond), "dx": …, "towers": [(dW, db)…
    flattened tower-major, hidden layers then the output layer]}; a None bias has no entry."""
    x, towers = leaves(x, dtype), leaves(towers, dtype)
    keeps = None if keeps is None else {s: k.to(dtype) for s, k in keeps.items()}
    out = esmm(x, towers, keeps, ordered)
    B, K = out[0].shape
    loss = torch.zeros((), dtype=dtype)
    for name, c, o in zip(("probs", "logits", "cond"), loss_coeffs(B, K), out):
        if name in use:
            loss = loss + (c.to(dtype) * o).sum()
    loss.backward()
    zero = lambda ts: [t.grad if t.grad is not None else torch.zeros_like(t) for t in ts]  # noqa: E731
    return dict(out=tuple(o.detach() for o in out), dx=zero([x])[0], towers=zero(flat(towers)))


def model_gradients(p, dense, category, dtype=torch.float64, keeps=None, ordered=False):
    """(probs, logits, {state_dict key: gradient}) of the model-level loss sum(c_p probs) + sum(c_l logits)."""
    q = {k: (v.detach().to(dtype).clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in p.items()}
    keeps = None if keeps is None else {s: k.to(dtype) for s, k in keeps.items()}
    probs, logits = forward(q, dense, category, keeps, ordered)
    cp, cl, _ = (c.to(dtype) for c in loss_coeffs(*logits.shape))
    ((cp * probs).sum() + (cl * logits).sum()).backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in q.items() if v.is_floating_point()}
    return probs.detach(), logits.detach(), grads


def joint_gradients(z, use=("probs", "logits", "cond"), dtype=torch.float64):
    """(the incoming gradients {name: [B, K]} in `use`, d/dz of sum_name sum(c_name * output_name(z))) by autograd
    of esmm_ref.chain: what rk_esmm_joint_backward folds."""
    z = z.detach().to(dtype).clone().requires_grad_(True)
    probs, cond = R.chain(z)
    coeffs = dict(zip(("probs", "logits", "cond"), loss_coeffs(*z.shape)))
    loss = torch.zeros((), dtype=dtype)
    for name, o in (("probs", probs), ("logits", z), ("cond", cond)):
        if name in use:
            loss = loss + (coeffs[name].to(dtype) * o).sum()
    loss.backward()
    return {n: coeffs[n] for n in use}, z.grad


def group_of(key):
    """The tolerance group (0 dx, 1 dw) of a state_dict key."""
    return 0 if key.startswith("embeddings.") else 1


def sites_of(K, tu):
    """[(site, n)…] of a configuration."""
    return [(k * len(tu) + l, tu[l]) for k in range(K) for l in range(len(tu))]


def op_inputs(c):
    return R.op_inputs(c)


_REFS = {}


def op_reference(c):
    """float64 outputs and gradients of one op-level case (all three outputs in the loss), computed once."""
    if c[0] not in _REFS:
        rows, towers = op_inputs(c)
        _REFS[c[0]] = op_gradients(rows[:, :c[1]], towers)
    return _REFS[c[0]]


def build_model(kw, seed=42, **flags):
    """Seeded rankops.ESMM on the small vocabulary (CPU, train mode untouched), heads scaled as esmm_ref's."""
    return R.build_model(("m", "small", 0, kw), seed, **flags)


def model_inputs(B, seed=1000):
    """(dense [B, 16], category {field: [B]}) on the small vocabulary."""
    import helpers as Hh
    inp = Hh.dcn_inputs(B, Hh.SMALL_VOCAB, seed)
    return inp["dense"], inp["category"]


def drifts():
    """[dx, dw, joint]: float32 (ordered) against float64 gradient drift."""
    out = [0.0, 0.0, 0.0]

    def upd(i, a, b):
        out[i] = max(out[i], R.rel_err(a, b))
    for c in GRAD_CASES:
        rows, towers = op_inputs(c)
        ref = op_reference(c)
        got = op_gradients(rows[:, :c[1]], towers, torch.float32, ordered=True)
        upd(0, got["dx"], ref["dx"])
        for a, b in zip(got["towers"], ref["towers"]):
            upd(1, a, b)
    for name, B, kw in MODEL_CASES:
        p = build_model(kw).state_dict()
        dense, cat = model_inputs(B)
        K = 2 if not kw else len(kw["task_names"])
        tu = kw.get("tower_hidden_units", (256, 128, 64))
        keeps = cpu_keeps(sites_of(K, tu), B, DROPOUT_P)
        _, _, ref = model_gradients(p, dense, cat, keeps=keeps)
        _, _, got = model_gradients(p, dense, cat, torch.float32, keeps=keeps, ordered=True)
        for k in ref:
            upd(group_of(k), got[k], ref[k])
    for lc in R.LOSS_CASES:
        z = R.loss_inputs(lc)[0][:, :lc[1]]
        upd(2, joint_gradients(z, dtype=torch.float32)[1], joint_gradients(z)[1])
    return out


if __name__ == "__main__":
    for n, v in zip(("dx", "dw", "joint"), drifts()):
        print(f"{n:6s} drift {v:.2e}  ->  {50 * v:.1e}")
