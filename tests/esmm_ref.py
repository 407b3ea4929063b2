"""Restatement of ESMM (rankops.ESMM's definition: Ma et al., SIGIR 2018, in rankops.MMoE's conventions)
in plain torch, in the dtype of its inputs (the tests run it in float64), the entire-space loss with its
analytic gradient as rk_esmm_loss formulates them, plus the seeded inputs and the tolerances of
tests/test_gpu_esmm.py and the loss tests of tests/test_gpu_esmm_train.py.

Tolerances.  A tolerance t is used as |got - ref| <= t * (1 + |ref|) against the float64 restatement
(`rel_err`, mmoe_ref's).  Each is 50 x the drift of this same restatement run in float32 against float64,
drift = max |f32 - f64| / (1 + |f64|) over the seeded inputs of the GPU tests: every ordinary op-level
case and the model-level cases for logits, probabilities and conditionals; the loss cases of logit scale 2
for the loss, the per-task means and the gradient.  The gradient is compared as B * dlogits (the per-row
gradient, of order 1 whatever the batch).  The `saturated` op case (head weights x SAT_SCALE: logits of
magnitude 20-30 in both signs, joint probabilities within 1e-6 of 0 and of 1) and the loss cases of logit
scale 8 (N(0, 8^2) logits clipped to +-30) have their own constants from their own drift, so that they do
not loosen the others.  tests/test_esmm_ref.py measures the drifts again and fails if a constant lies
outside 25-100 x of what it measures.  The float32 forward takes every sum in a fixed order
(`ordered=True`, see mmoe_ref.linear).  Measured (torch 2.x, CPU):

    ordinary   logits drift 4.60e-07  ->  LOGIT_TOL 2.3e-05
               probs  drift 1.08e-07  ->  PROB_TOL  5.4e-06
               cond   drift 6.73e-08  ->  COND_TOL  3.4e-06
    saturated  logits drift 1.45e-06  ->  SAT_LOGIT_TOL 7.3e-05
               probs  drift 4.29e-07  ->  SAT_PROB_TOL  2.1e-05
               cond   drift 4.20e-07  ->  SAT_COND_TOL  2.1e-05
    loss, scale 2   loss drift 3.62e-08 -> LOSS_TOL 1.8e-06; per task 2.70e-08 -> TASK_LOSS_TOL 1.3e-06;
                    B * dlogits 1.28e-07 -> DLOGIT_TOL 6.4e-06
    loss, scale 8   loss drift 1.57e-08 -> SAT_LOSS_TOL 7.9e-07; per task 4.91e-08 -> SAT_TASK_LOSS_TOL 2.5e-06;
                    B * dlogits 1.37e-07 -> SAT_DLOGIT_TOL 6.9e-06
"""
from __future__ import annotations

import math

import torch

import mmoe_ref as M
from mmoe_ref import cast, floats, model_row, rel_err, vocab  # noqa: F401

LOGIT_TOL = 2.3e-05
PROB_TOL = 5.4e-06
COND_TOL = 3.4e-06
SAT_LOGIT_TOL = 7.3e-05
SAT_PROB_TOL = 2.1e-05
SAT_COND_TOL = 2.1e-05
LOSS_TOL = 1.8e-06
TASK_LOSS_TOL = 1.3e-06
DLOGIT_TOL = 6.4e-06
SAT_LOSS_TOL = 7.9e-07
SAT_TASK_LOSS_TOL = 2.5e-06
SAT_DLOGIT_TOL = 6.9e-06

# (name, width, K, tower units, B): the smallest shapes at which rk_esmm_forward can still go wrong (the
# default shape with a ragged last tile, one live row, 16 + 1 rows, widths off the 16 grid over an odd
# input width, the 512-wide two-tile path over 13 input chunks, the longest chain, saturated logits)
OP_CASES = [
    ("wechat", 50, 2, (256, 128, 64), 300),
    ("one_row", 50, 2, (256, 128, 64), 1),
    ("tile_edge", 50, 2, (64,), 17),
    ("odd", 37, 3, (24, 7), 33),
    ("wide", 200, 4, (512, 100, 40), 16),
    ("chain8", 50, 8, (16,), 20),
    ("saturated", 50, 3, (32,), 64),
]
SATURATED = "saturated"
ROW_PAD = 6        # the op-level rows lie in a buffer with row stride width + ROW_PAD
X_STD = 0.7        # spread of the op-level input rows
HEAD_SCALE = 4.0   # ordinary cases: head weights and biases at 4 x nn.Linear's init range, so that the
                   # conditionals are spread over (0, 1) and the towers' logits differ
SAT_SCALE = 60.0   # `saturated`: logits of magnitude 20-30 in both signs

# model-level cases: (name, vocab ("small" | "wechat"), batch, constructor arguments)
ALT_CONFIG = dict(tower_hidden_units=(64,), task_names=("click", "cart", "purchase"))
MODEL_CASES = [
    ("small_default", "small", 300, {}),
    ("small_alt", "small", 300, ALT_CONFIG),
    ("wechat_default", "wechat", 257, {}),
    ("wechat_alt", "wechat", 257, ALT_CONFIG),
]

# loss cases: (B, K, logit scale, task weights or None).  (5000, 2, 8) gives rk_esmm_loss more than one
# workgroup and a ragged last one in the reduction.
LOSS_CASES = [(1, 2, 2.0, None), (17, 2, 2.0, None), (300, 3, 8.0, (1.0, 0.5, 2.0)), (5000, 2, 8.0, None),
              (64, 8, 2.0, None)]
LOSS_PAD = 3       # logits and labels lie in buffers with row stride K + LOSS_PAD
LOGIT_CLIP = 30.0


def case(name):
    return next(c for c in OP_CASES if c[0] == name)


def tolerances(name):
    """(logits, probs, cond) tolerances of an op-level case."""
    if name == SATURATED:
        return SAT_LOGIT_TOL, SAT_PROB_TOL, SAT_COND_TOL
    return LOGIT_TOL, PROB_TOL, COND_TOL


def loss_tolerances(scale):
    """(loss, per-task, B * dlogits) tolerances of a loss case."""
    if scale > 4:
        return SAT_LOSS_TOL, SAT_TASK_LOSS_TOL, SAT_DLOGIT_TOL
    return LOSS_TOL, TASK_LOSS_TOL, DLOGIT_TOL


# ---------------------------------------------------------------- the definition

def chain(logits):
    """(probs, cond): cond = sigmoid(logits), probs the cumulative product taken k ascending."""
    cond = torch.sigmoid(logits)
    cols, run = [], None
    for k in range(logits.shape[1]):
        run = cond[:, k] if run is None else run * cond[:, k]
        cols.append(run)
    return torch.stack(cols, dim=1), cond


def esmm(x, towers, clipped=None, ordered=False):
    """x [B, width]; towers: K (hidden [(W, b)…], (w_out [1, ·], b_out or None)).  Returns (probs, logits,
    cond), each [B, K].  ordered: every sum in a fixed order (mmoe_ref.linear)."""
    logits = []
    for hidden, (w_out, b_out) in towers:
        t = M.stack(x, hidden, clipped, ordered)
        logits.append(M.linear(t, w_out.reshape(1, -1), None if b_out is None else b_out.reshape(1, 1), ordered))
    logits = torch.cat(logits, dim=1)
    probs, cond = chain(logits)
    return probs, logits, cond


def model_parts(p):
    """towers of a rankops.ESMM state_dict, in esmm()'s form."""
    tw = M._layout(p, "towers.")
    return [([(p[f"towers.{k}.{i}.weight"], p[f"towers.{k}.{i}.bias"]) for i in tw[k]],
             (p[f"tower_outputs.{k}.weight"], p[f"tower_outputs.{k}.bias"])) for k in sorted(tw)]


def forward(p, dense, category, keep=None, ordered=False):
    """(probabilities [B, K], logits [B, K]) of a rankops.ESMM state_dict, in p's dtype."""
    probs, logits, _ = esmm(model_row(p, dense, category, keep), model_parts(p), ordered=ordered)
    return probs, logits


# ---------------------------------------------------------------- the entire-space loss

def log1mexp(s):
    """log(1 - exp(s)) for s < 0: log(-expm1(s)) for s > -ln 2, else log1p(-exp(s))."""
    near = s > -math.log(2.0)
    return torch.where(near, torch.log(-torch.expm1(torch.where(near, s, torch.full_like(s, -1.0)))),
                       torch.log1p(-torch.exp(torch.where(near, torch.full_like(s, -1.0), s))))


def tree_sum(L):
    """Column sums of L [B, K] as a fixed pairwise tree of element-wise additions (zero rows up to a power
    of two), so that the float32 sum is the same number on every machine (torch's own sum is not)."""
    n = 1
    while n < L.shape[0]:
        n *= 2
    L = torch.cat([L, torch.zeros(n - L.shape[0], L.shape[1], dtype=L.dtype)], dim=0)
    while n > 1:
        n //= 2
        L = L[:n] + L[n:]
    return L[0]


def loss(z, y, w=None):
    """The entire-space loss over conditional logits z [B, K] and joint labels y [B, K], as rk_esmm_loss
    formulates it (include/rankops.h), with its analytic gradient, in z's dtype: (loss, per-task means [K],
    dlogits [B, K] = d loss / d z)."""
    B, K = z.shape
    tiny = torch.finfo(torch.float32).tiny
    w = torch.ones(K, dtype=z.dtype) if w is None else torch.as_tensor(w, dtype=z.dtype)
    sp = torch.nn.functional.softplus
    ls = -sp(-z)                                                   # logsigmoid
    sn = torch.sigmoid(-z)
    L = [sp(-z[:, 0]) * y[:, 0] + sp(z[:, 0]) * (1 - y[:, 0])]
    S, coef = ls[:, 0], [None]
    for k in range(1, K):
        S = S + ls[:, k]
        Sc = torch.clamp(S, max=-tiny)
        L.append(-(y[:, k] * S + (1 - y[:, k]) * log1mexp(Sc)))
        coef.append(((1 - y[:, k]), torch.expm1(-Sc), y[:, k]))
    per_task = tree_sum(torch.stack(L, dim=1)) / B
    g = torch.zeros_like(z)
    g[:, 0] = (torch.sigmoid(z[:, 0]) - y[:, 0]) * w[0]
    for j in range(K):
        for k in range(max(j, 1), K):
            one_minus_y, em, yk = coef[k]
            g[:, j] = g[:, j] + w[k] * ((sn[:, j] * one_minus_y) / em - sn[:, j] * yk)
    return (per_task * w).sum(), per_task, g / B


def loss_inputs(lc, seed=11):
    """float32 CPU (logit buffer, label buffer) of a loss case, each [B, K + LOSS_PAD]: logits N(0, scale^2)
    clipped to +-LOGIT_CLIP in the first K columns, nested labels y_k <= y_{k-1} there."""
    B, K, scale, _ = lc
    g = torch.Generator().manual_seed(seed + 7 * B + 131 * K + int(scale))
    zb = torch.randn(B, K + LOSS_PAD, generator=g)
    zb[:, :K] = (zb[:, :K] * scale).clamp(-LOGIT_CLIP, LOGIT_CLIP)
    yb = torch.rand(B, K + LOSS_PAD, generator=g)
    y = (yb[:, :K] < 0.6).float()
    yb[:, :K] = torch.cumprod(y, dim=1)
    return zb, yb


_LOSS_REFS = {}


def loss_reference(lc):
    """float64 (loss, per-task, dlogits) of a loss case, computed once (do not modify it)."""
    if lc not in _LOSS_REFS:
        zb, yb = loss_inputs(lc)
        K = lc[1]
        _LOSS_REFS[lc] = loss(zb[:, :K].double(), yb[:, :K].double(), lc[3])
    return _LOSS_REFS[lc]


# ---------------------------------------------------------------- seeded inputs of the GPU tests

# Seeds chosen so that every case meets the conditions tests/test_esmm_ref.py asserts (towers that differ,
# factors that move the product, no dead layer, saturation in both directions)
CASE_SEEDS = {}


def op_inputs(c, seed=None):
    """float32 CPU inputs of one op-level case: the row buffer [B, width + ROW_PAD] (x = its first `width`
    columns) and towers in esmm()'s form."""
    name, width, K, tu, B = c
    seed = CASE_SEEDS.get(name, 2025) if seed is None else seed
    g = torch.Generator().manual_seed(seed + 131 * width + 7 * K + B + 3 * len(tu))
    rows = torch.randn(B, width + ROW_PAD, generator=g) * X_STD
    scale = SAT_SCALE if name == SATURATED else HEAD_SCALE
    towers = []
    for _ in range(K):
        hidden, last = M._stack_inputs(g, width, tu)
        towers.append((hidden, M._linear(g, 1, last, scale)))
    return rows, towers


_REFS = {}


def op_reference(c, dtype=torch.float64, clipped=None, ordered=False):
    """(probs, logits, cond) of one op-level case from the restatement in `dtype`; the float64 result is
    computed once and shared (do not modify it)."""
    key = (c[0], dtype, ordered)
    if clipped is None and key in _REFS:
        return _REFS[key]
    rows, towers = op_inputs(c)
    out = esmm(rows[:, :c[1]].to(dtype), cast(towers, dtype), clipped, ordered)
    if clipped is None:
        _REFS[key] = out
    return out


def build_model(mc, seed=42, **flags):
    """Seeded rankops.ESMM (CPU, eval) of a model case, its head weights and biases x HEAD_SCALE."""
    import rankops
    _, which, _, kw = mc
    torch.manual_seed(seed)
    model = rankops.ESMM(None, vocab_sizes=vocab(which), **kw, **flags)
    with torch.no_grad():
        for head in model.tower_outputs:
            head.weight.mul_(HEAD_SCALE)
            head.bias.mul_(HEAD_SCALE)
    return model.eval()


def model_inputs(mc, seed=1000):
    import helpers as H
    _, which, B, _ = mc
    return H.dcn_inputs(B, vocab(which), seed)


def drifts():
    """{"ordinary": [logits, probs, cond], "saturated": […], "loss": [loss, per task, B dlogits], "sat_loss": […]}:
    the float32 (ordered) restatement's drift against float64."""
    import helpers as H
    out = {"ordinary": [0.0] * 3, "saturated": [0.0] * 3, "loss": [0.0] * 3, "sat_loss": [0.0] * 3}

    def upd(which, i, a, b):
        out[which][i] = max(out[which][i], rel_err(a, b))
    for c in OP_CASES:
        ref = op_reference(c)
        got = op_reference(c, torch.float32, ordered=True)
        which = "saturated" if c[0] == SATURATED else "ordinary"
        for i, j in enumerate((1, 0, 2)):
            upd(which, i, got[j], ref[j])
    for mc in MODEL_CASES:
        p = H.cpu_params(build_model(mc))
        inp = model_inputs(mc)
        ref = forward(floats(p, torch.float64), **inp)
        got = forward(p, ordered=True, **inp)
        upd("ordinary", 0, got[1], ref[1])
        upd("ordinary", 1, got[0], ref[0])
    for lc in LOSS_CASES:
        B, K, scale, w = lc
        zb, yb = loss_inputs(lc)
        ref = loss_reference(lc)
        got = loss(zb[:, :K], yb[:, :K], w)
        which = "sat_loss" if scale > 4 else "loss"
        upd(which, 0, got[0], ref[0])
        upd(which, 1, got[1], ref[1])
        upd(which, 2, got[2] * B, ref[2] * B)
    return out


if __name__ == "__main__":
    for which, d in drifts().items():
        names = ("loss", "task", "B dz") if "loss" in which else ("logits", "probs", "cond")
        for n, v in zip(names, d):
            print(f"{which:9s} {n:6s} drift {v:.2e}  ->  {50 * v:.1e}")
