"""Restatement of xDeepFM's training step for tests/test_gpu_xdeepfm_train.py: tests/xdeepfm_ref.py's
CIN and model differentiated by torch autograd, in the dtype of the inputs (the tests run float64).

ReLU mask.  The CIN's ReLU takes an optional 0/1 mask per layer, x^k = y^k * mask_k, so the reference
can differentiate with the activation pattern the engine saw (its own maps > 0): where a
pre-activation is within rounding of zero the two sides may legitimately disagree on its sign, and a
gradient through torch.relu would then differ by a whole term.  With mask = (y^k > 0) the masked form
is torch.relu, value and gradient (tests/test_xdeepfm_train_ref.py).

Op-level loss: (pooled * G).sum() + (logit * g).sum() with seeded G [B, sum H_k], g [B, 1].

GRAD_TOL.  A gradient tensor is compared as max |got - want| <= GRAD_TOL * max |want| (a tensor whose
reference is all zero must be exactly zero).  The constant is 50 x the drift of this restatement run in
float32 against float64, drift = max |f32 - f64| / max |f64| per gradient tensor (dx0, every dW_k and
dbias_k, d out_w, d out_b) over xdeepfm_ref.OP_CASES with both activations and the full loss; 50 x is
the project's margin for another summation order on MFMA (tests/xdeepfm_ref.py).
tests/test_xdeepfm_train_ref.py measures the drift again and fails if the constant leaves 25-100 x.
Measured on the CPU (torch 2.x, float32):

    largest drift 8.17e-07 (dW_1 of wide_k, identity)  ->  GRAD_TOL 4.1e-05

SLAB_CASE (the reduction-slab test, B 1,000) is compared with the same constant but takes no part in
deriving it: its float32 drift on the CPU depends on how many threads torch splits the 8,000-long
reduction of dW over (8.2e-7 measured with 8 threads, 2.0e-6 with 16), so it would make the constant a
property of the host.  A longer reduction can only raise the drift, so the constant from the short
cases is the stricter bound for it.

NEAR_KINK_MAX caps the share of ReLU pre-activations with |y| <= POOLED_TOL * (1 + |y|), the band in
which the engine's sign may differ from the reference's: measured <= 2.4e-4 per case.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

import xdeepfm_ref as X
from oracle import reference_forward as ref

GRAD_TOL = 4.1e-05
NEAR_KINK_MAX = 1e-3
# the wechat shape at a batch that spans every slab of the weight-gradient kernel (32 slabs of four
# 8-sample tiles, the last slab one tile)
SLAB_CASE = ("wechat_b1000", 6, 8, (128, 128), 1000)
GPU_OP_CASES = X.OP_CASES + [SLAB_CASE]


def cin(x0, Ws, bs, act="identity", masks=None):
    """xdeepfm_ref.cin with the ReLU as a product with masks[k] [B, H_k, D] when given.
    Returns (pooled [B, sum H_k], maps [x^k], pre-activations [y^k])."""
    B, m, D = x0.shape
    xk, pooled, maps, pre = x0, [], [], []
    for k, (W, b) in enumerate(zip(Ws, bs)):
        z = (xk.unsqueeze(2) * x0.unsqueeze(1)).reshape(B, xk.shape[1] * m, D)  # z[b, h m + i, d]
        y = torch.matmul(W.reshape(W.shape[0], -1), z) + b.view(1, -1, 1)
        if act == "identity":
            xk = y
        elif masks is not None:
            xk = y * masks[k].to(y.dtype)
        else:
            xk = torch.relu(y)
        pre.append(y)
        maps.append(xk)
        pooled.append(xk.sum(dim=2))
    return torch.cat(pooled, dim=1), maps, pre


def loss_weights(case, seed=77):
    """The seeded G [B, sum H_k] and g [B, 1] of the op-level loss."""
    _, m, D, sizes, B = case
    gen = torch.Generator().manual_seed(seed + 7 * m + D + B)
    return torch.randn(B, sum(sizes), generator=gen), torch.randn(B, 1, generator=gen)


GRAD_NAMES = ("dx0", "dW", "dbias", "dout_w", "dout_b")


def op_grads(case, act, dtype=torch.float64, masks=None, output_layer=True):
    """One op-level case differentiated by autograd: dict with pooled, logit, maps, pre and the
    gradients dx0 [B, m, D], dW [per layer], dbias [per layer], dout_w, dout_b (None without the
    output layer) of loss = (pooled * G).sum() + (logit * g).sum()."""
    _, m, D, _, B = case
    rows, Ws, bs, out_w, out_b = X.op_inputs(case)
    G, g = loss_weights(case)
    x0 = rows[:, :m * D].reshape(B, m, D).to(dtype).requires_grad_(True)
    Ws = [w.to(dtype).requires_grad_(True) for w in Ws]
    bs = [b.to(dtype).requires_grad_(True) for b in bs]
    out_w, out_b = out_w.to(dtype).requires_grad_(True), out_b.to(dtype).requires_grad_(True)
    pooled, maps, pre = cin(x0, Ws, bs, act, masks)
    loss = (pooled * G.to(dtype)).sum()
    logit = None
    if output_layer:
        logit = pooled @ out_w.view(-1, 1) + out_b
        loss = loss + (logit * g.to(dtype)).sum()
    loss.backward()
    return dict(pooled=pooled.detach(), logit=None if logit is None else logit.detach(),
                maps=[t.detach() for t in maps], pre=[t.detach() for t in pre], dx0=x0.grad,
                dW=[w.grad for w in Ws], dbias=[b.grad for b in bs],
                dout_w=out_w.grad if output_layer else None, dout_b=out_b.grad if output_layer else None)


def grad_tensors(r):
    """(name, tensor) of every gradient in an op_grads result."""
    out = [("dx0", r["dx0"])]
    out += [(f"dW_{k + 1}", t) for k, t in enumerate(r["dW"])]
    out += [(f"dbias_{k + 1}", t) for k, t in enumerate(r["dbias"])]
    if r["dout_w"] is not None:
        out += [("dout_w", r["dout_w"]), ("dout_b", r["dout_b"])]
    return out


def grad_err(got, want):
    """max |got - want| / max |want|: the quantity GRAD_TOL bounds (want not all zero)."""
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


def near_kink(y, tol=X.POOLED_TOL):
    """The band around zero in which a pre-activation's sign is not decided at the forward's tolerance."""
    return y.abs() <= tol * (1 + y.abs())


def forward_train(p, category, cin_activation="identity", cin_masks=None, num_hidden=3, batch_norm=True,
                  dropout_rate=0.1, masks=None, momentum=0.1, eps=1e-5):
    """XDeepFM.forward in model.train(): xdeepfm_ref.forward's front (first-order sum, CIN with the given
    ReLU masks, cin_output_layer) and the tail of the oracle's deepfm_forward_train (BatchNorm1d with
    batch statistics, running statistics in `p` updated in place, Dropout as the given multiplier
    masks) with the FM term replaced by cin_logit; differentiable w.r.t. the tensors in `p`."""
    fields = [k.split(".")[1] for k in p if k.startswith("second_order_embeddings.")]
    first = [F.embedding(category[c], p[f"first_order_embeddings.{c}.weight"]) for c in fields]
    linear = torch.sum(torch.cat(first, dim=1), dim=1, keepdim=True)
    second = [F.embedding(category[c], p[f"second_order_embeddings.{c}.weight"]) for c in fields]
    x0 = torch.stack(second, dim=1)
    nl = len([k for k in p if k.startswith("cin_layers.") and k.endswith(".weight")])
    pooled, _, _ = cin(x0, [p[f"cin_layers.{k}.weight"] for k in range(nl)],
                       [p[f"cin_layers.{k}.bias"] for k in range(nl)], cin_activation, cin_masks)
    cin_logit = F.linear(pooled, p["cin_output_layer.weight"], p["cin_output_layer.bias"])
    h = torch.cat(second, dim=1)
    for u, (lin, bn) in enumerate(ref.deepfm_layout(num_hidden, batch_norm, dropout_rate)):
        h = ref._lin(h, p, f"deep_layers.{lin}.")
        if bn is not None:
            pre = f"deep_layers.{bn}."
            h = F.batch_norm(h, p[pre + "running_mean"], p[pre + "running_var"], p[pre + "weight"], p[pre + "bias"],
                             training=True, momentum=momentum, eps=eps)
            p[pre + "num_batches_tracked"] += 1
        h = torch.relu(h)
        if masks is not None and masks[u] is not None:
            h = h * masks[u]
    deep = ref._lin(h, p, "deep_output_layer.")
    total = ref._lin(torch.cat([linear, cin_logit, deep], dim=1), p, "final_layer.")
    return torch.sigmoid(total), total, linear, cin_logit, deep
