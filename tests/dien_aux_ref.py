"""Restatement of DIEN's auxiliary loss in plain torch ops, on top of the extractor states
dien_ref.interest returns.  A helper, not a test: float64 on the CPU is the oracle of
tests/test_dien_aux_host.py and tests/test_gpu_dien_aux.py.

Written from the reference block (algorithm/DIEN/dien.py:256-300: project with aux_project_matrix
[na, nh], dot every h_t with the next behaviour and with T_neg negatives, mask by
sequence_mask(length - 1, T - 1), sum, batch mean), with its two defects corrected: the positives
are the embedded history shifted by one step (dien.py:265 slices the length tensor), and the sign
is the paper's, L_aux = -mean_b sum_t [log sig(pos) + sum_n log(1 - sig(neg))] (dien.py:300,317
adds the bracket itself, which training would maximise).  log sig(x) is computed as
min(x, 0) - log1p(exp(-|x|)): the reference's own note blames tf.log for inf / nan.

Negatives: [B, (T-1) * T_neg, H], entry t * T_neg + n pairs with h_t (the reference's reshape to
(B, T-1, T_neg, nh), dien.py:279).  All T_neg are used, as the reference does.

REL_LOSS / REL_GRAD are the relative tolerances of the GPU tests (atol = REL * max|want|, rtol 0):
50 times the worst fp32-vs-fp64 drift of this restatement, measured and asserted by
test_dien_aux_host.py::test_tolerances_are_fifty_times_the_fp32_drift (figures in its docstring).
"""
from __future__ import annotations

import functools

import torch

import dien_ref

REL_LOSS = 2.0e-5
REL_GRAD = 1.0e-4
VOCAB = 301
SHAPES = [(1, 1, 16, 8), (1, 2, 16, 8), (3, 3, 8, 8), (9, 17, 32, 8), (67, 50, 16, 8), (5, 200, 32, 16)]
CELLS = ("AGRU", "AUGRU")
T_NEGS = (1, 3)


def log_sigmoid(x):
    return torch.clamp(x, max=0) - torch.log1p(torch.exp(-x.abs()))


def aux_loss(hs, keys, neg, lengths, w_aux, dtype=torch.float64):
    """hs [B,T,nh], keys [B,T,H], neg [B,(T-1)*T_neg,H], lengths [B], w_aux [H,nh]
    -> (mean over the batch, per-sample [B])."""
    hs, keys, neg, w_aux = hs.to(dtype), keys.to(dtype), neg.to(dtype), w_aux.to(dtype)
    B, T, H = keys.shape
    if T == 1:
        per = (hs.sum((1, 2)) + keys.sum((1, 2)) + w_aux.sum()) * 0  # exactly zero, still attached to the leaves
        return per.mean(), per
    T_neg = neg.shape[1] // (T - 1)
    g = hs[:, :-1] @ w_aux.T                                   # [B, T-1, H]: W_aux h_t
    pos = (g * keys[:, 1:]).sum(-1)                            # [B, T-1]
    negd = torch.einsum("bth,btnh->btn", g, neg.reshape(B, T - 1, T_neg, H))
    mask = (torch.arange(T - 1, device=keys.device)[None, :] < (lengths.to(keys.device)[:, None] - 1)).to(dtype)
    term = log_sigmoid(pos) + log_sigmoid(-negd).sum(-1)
    per = -(term * mask).sum(1)
    return per.mean(), per


def aux_loss_loop(hs, keys, neg, lengths, w_aux):
    """The same, one Python step per (b, t, n), float64: the formulae read off one by one."""
    hs, keys, neg, w_aux = hs.double(), keys.double(), neg.double(), w_aux.double()
    B, T, H = keys.shape
    T_neg = neg.shape[1] // (T - 1) if T > 1 else 0
    per = torch.zeros(B, dtype=torch.float64)
    for b in range(B):
        for t in range(max(0, min(int(lengths[b]), T) - 1)):
            g = w_aux @ hs[b, t]
            total = log_sigmoid(g @ keys[b, t + 1])
            for n in range(T_neg):
                total = total + log_sigmoid(-(g @ neg[b, t * T_neg + n]))
            per[b] = per[b] - total
    return per.mean() if B else per.sum(), per


def aux_loss_reference_form(hs, keys, neg, lengths, w_aux):
    """dien.py:268-300 line by line in float64 (project the rows, log(sigmoid), log(1 - sigmoid), the
    two masks, reduce), with sequnence_input where the reference slices sequnence_length, and the
    sign flipped.  Only for mild inputs: this form is the one that overflows."""
    hs, keys, neg, w_aux = hs.double(), keys.double(), neg.double(), w_aux.double()
    B, T, H = keys.shape
    T_neg = neg.shape[1] // (T - 1)
    h_ = hs[:, :-1]
    pos = keys[:, 1:] @ w_aux
    negp = (neg @ w_aux).reshape(B, T - 1, T_neg, -1)
    pos_part = torch.log(torch.sigmoid(torch.einsum("bth,bth->bt", h_, pos)))
    neg_part = torch.log(1 - torch.sigmoid(torch.einsum("bth,btnh->btn", h_, negp)))
    aux_mask = (torch.arange(T - 1)[None, :] < (lengths[:, None] - 1)).double()
    pos_part = (pos_part * aux_mask).sum(1, keepdim=True)
    neg_part = (neg_part * aux_mask[:, :, None]).sum((1, 2)).unsqueeze(-1)
    return -(pos_part + neg_part).mean()


def forced_lengths(B, T, lens):
    """Lengths T, 2, 1, 0 in the first samples (as many as the batch has)."""
    forced = torch.tensor([T, min(2, T), 1, 0])[:B]
    lens = lens.clone()
    lens[:len(forced)] = forced
    return lens


@functools.lru_cache(maxsize=None)
def case(B, T, Hd, nh, T_neg, seed=23):
    """Seeded op inputs (CPU), shared by every test of the shape and never modified:
    (query, table, ids, neg_ids, lengths, interest weights, w_aux, upstream G [B, nh])."""
    g = torch.Generator().manual_seed(seed + 13 * B + T + 101 * T_neg)
    q = torch.randn(B, Hd, generator=g)
    table = torch.randn(VOCAB, Hd, generator=g)
    ids = torch.randint(0, VOCAB, (B, T), generator=g)
    neg_ids = torch.randint(0, VOCAB, (B, (T - 1) * T_neg), generator=g)
    lens = forced_lengths(B, T, torch.randint(0, T + 1, (B,), generator=g))
    w_aux = (torch.rand(Hd, nh, generator=g, dtype=torch.float64) - 0.5).float()
    G = torch.randn(B, nh, generator=g)
    return q, table, ids, neg_ids, lens, tuple(dien_ref.draw_weights(Hd, nh, seed + 1)), w_aux, G


OP_NAMES = ("d_hs", "dkeys", "dneg", "dw_aux")
COMP_NAMES = ("dq", "dkeys", "dneg") + tuple("d" + n for n in dien_ref.WEIGHT_NAMES) + ("dw_aux",)


@functools.lru_cache(maxsize=None)
def op_oracle(B, T, Hd, nh, T_neg, cell, dtype=torch.float64):
    """The loss alone on the restatement's own states (rounded to float32, the tensor the kernels are
    fed): (hs float32, mean, per_sample, gradients in OP_NAMES order)."""
    q, table, ids, neg_ids, lens, w, w_aux, _ = case(B, T, Hd, nh, T_neg)
    with torch.no_grad():
        hs = dien_ref.interest(q, table[ids], lens, w, cell)[2].float()
    leaves = [t.detach().clone().to(dtype).requires_grad_(True) for t in (hs, table[ids], table[neg_ids], w_aux)]
    mean, per = aux_loss(*leaves[:3], lens, leaves[3], dtype=dtype)
    mean.backward()
    return hs, mean.detach(), per.detach(), tuple(t.grad for t in leaves)


@functools.lru_cache(maxsize=None)
def composition_oracle(B, T, Hd, nh, T_neg, cell, dtype=torch.float64):
    """(state * G).sum() / B + aux_loss(hs, ...) through dien_ref.interest: (loss, gradients in
    COMP_NAMES order)."""
    q, table, ids, neg_ids, lens, w, w_aux, G = case(B, T, Hd, nh, T_neg)
    leaves = [t.detach().clone().to(dtype).requires_grad_(True) for t in (q, table[ids], table[neg_ids], *w, w_aux)]
    state, _, hs = dien_ref.interest(leaves[0], leaves[1], lens, leaves[3:12], cell, dtype=dtype)
    loss = (state * G.to(dtype)).sum() / B + aux_loss(hs, leaves[1], leaves[2], lens, leaves[12], dtype=dtype)[0]
    loss.backward()
    return loss.detach(), tuple(t.grad for t in leaves)
