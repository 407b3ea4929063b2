"""DIEN (Deep Interest Evolution Network) on the rankops engine — the model of algorithm/DIEN/dien.py
(a TF1 Estimator there; it does not run, so this is its mathematics, not a line-for-line port).

`DIEN(vocab_dir, hidden_units=None, activation='dice', dropout_rate=0.1, batch_norm=True,
custom_gru_type='AGRU', gru_output_units=8)` takes the reference's flags (dien.py:40-53) and
`forward(dense, category, sequence, target) -> (probability, logit)` the input dictionaries of
`rankops.DIN`.  Training is opt-in: `DIEN(..., trainable=True)` in `model.train()` returns outputs
attached to `rankops.train._DIENTrain` (HIP backward of the recurrence, dien.py:314-334's loop works
with `rankops.Adam`); a default-constructed model raises in train mode (common.check_eval).

The auxiliary loss (dien.py:256-300; flags `use_auxiliary_loss=False`, `negative_sample_number=3`,
keyword-only here) supervises every extractor state h_t with the next behaviour and with sampled
negatives.  With the flag on, a training forward takes the negatives' ids in
`sequence['neg_his_read_comment_7d_seq']` [B, (T-1)*negative_sample_number] (entry t*T_neg+n pairs
with step t; sampling is the caller's) and returns `(probability, logit, aux_loss)`; `loss = bce +
aux_loss` trains through HIP kernels end to end (rk_dien_aux_loss, rk_dien_aux_loss_backward,
rk_dien_interest_backward_aux).  The reference's block does not run; two of its defects are
corrected, not ported: it slices the length tensor where the embedded history is meant
(dien.py:265), and it adds mean(log sig(pos) + sum log(1 - sig(neg))) to the loss (dien.py:300,317),
the negative of the paper's L_aux; here the paper's sign is used, and log sig is computed as
min(x, 0) - log1p(exp(-|x|)).  Eval mode and a flag-off model are unchanged.  As functions:
`dien_interest(..., return_states=True)` hands out the states, `dien_aux_loss(_gather)` is the loss.

Parameters: `embeddings.*` as in DIN except that target and history share the one `feedid` table
(shared_embedding_columns, dien.py:126); `gru.gates` / `gru.candidate` (TF GRUCell: Linear(H+nh, 2nh)
with the reset rows first, Linear(H+nh, nh)); `attention_project_matrix` [nh, H];
`evolution.gates` / `evolution.candidate` (AGRU / AUGRU cell: Linear(2nh, 2nh), Linear(2nh, nh));
`fcn.*`, `output_layer.*` as in DIN.  Initialisation as TF does it: Glorot-uniform kernels, gate
biases 1 (custom_grucell.py:66-68), other biases 0.

Launches: the eval forward is one rk_dien_forward launch (common.FUSED_DIEN) inside its envelope
(gru_output_units 8, hidden units [512, 256, 128], a history short enough for 16 samples' rows in
LDS): the row [dense | category | target | .] is gathered into LDS, the interest recurrence (history
gather, GRU, attention scores, masked softmax, AGRU / AUGRU) writes the final interest state into
the row's last nh columns, and the fcn stack runs over it as DIN's tail.  Outside the envelope the
same three steps are three launches (rk_concat_gather, rk_dien_interest, the tail), with the same
bits.  `prepare(dense, category, sequence, target)` binds the one launch to its inputs like
DIN.prepare.  The row order is DIN's (dense in the given order, category in ModuleDict order), not
input_layer's alphabetical one: there is no TF checkpoint this could ever load.

Request-level scoring (eval, inference only): `extract_interests(sequence)` runs the interest
extractor over R histories once (rk_dien_extract), `score(dense, category, target, interests,
request_index)` runs attention, evolution and the tail for B candidates that name their request
(rk_dien_evolve); bit-equal to `forward` on the histories repeated per candidate.  As functions:
`dien_extract(_gather)`, `dien_evolve`.  `forward` keeps the one fused launch.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import common, ops, train
from .common import PACKED, EngineModule, Layer, check_eval, fused_mlp_fits, load_vocabulary, run_tail, table_rows
from .din import FIELDS, SEQ_KEY, Dice

NEG_SEQ_KEY = "neg_" + SEQ_KEY  # neg_his_read_comment_7d_seq: the auxiliary loss's sampled negatives
ENVELOPE = "H (embedding width) in {8, 16, 32}, nh (gru_output_units) in {8, 16}, 1 <= T <= 256"
WEIGHT_NAMES = ("Wg", "bg", "Wc", "bc", "A", "Vg", "vg", "Vc", "vc")


def _cell(cell_type) -> int:
    if cell_type not in ops.DIEN_CELLS:
        raise ValueError(f"rankops DIEN: custom_gru_type must be 'AGRU' or 'AUGRU', got {cell_type!r}")
    return ops.DIEN_CELLS[cell_type]


def _check_envelope(H: int, nh: int, T: int):
    if H not in (8, 16, 32) or nh not in (8, 16) or not 1 <= T <= 256:
        raise NotImplementedError(f"rankops dien_interest: H={H}, nh={nh}, T={T} is outside the kernel's envelope: "
                                  f"{ENVELOPE}")


def _weights(weights, H: int):
    """(Wg, bg, Wc, bc, A, Vg, vg, Vc, vc) checked against H and each other; returns them
    contiguous with nh."""
    if len(weights) != 9:
        raise ValueError(f"rankops dien_interest: weights must be {WEIGHT_NAMES}, got {len(weights)} tensors")
    ws = [ops.as_f32(w, f"weights[{n}]").contiguous() for n, w in zip(WEIGHT_NAMES, weights)]
    if ws[4].dim() != 2 or ws[4].shape[1] != H:
        raise ValueError(f"rankops dien_interest: A must be [nh, {H}], got {tuple(ws[4].shape)}")
    nh = ws[4].shape[0]
    want = ((2 * nh, H + nh), (2 * nh,), (nh, H + nh), (nh,), (nh, H), (2 * nh, 2 * nh), (2 * nh,), (nh, 2 * nh),
            (nh,))
    for n, w, shape in zip(WEIGHT_NAMES, ws, want):
        if tuple(w.shape) != shape:
            raise ValueError(f"rankops dien_interest: {n} must be {shape}, got {tuple(w.shape)}")
    return ws, nh


def _convert(rc_error, H, nh, T):
    if getattr(rc_error, "code", None) == ops._lib.RK_ERR_UNSUPPORTED:
        raise NotImplementedError(f"rankops dien_interest: H={H}, nh={nh}, T={T}: {rc_error}; envelope: "
                                  f"{ENVELOPE}") from rc_error
    raise rc_error


class _DIENInterest(torch.autograd.Function):
    """dien_interest / dien_interest_gather under autograd: rk_dien_interest_train(_dense) keeps the
    states, rk_dien_interest_backward gives dquery, dkeys and the nine weight gradients; the gather
    form scatters dkeys into a zeroed dense table gradient (rk_embedding_backward).  `keys` is the
    history [B,T,H] (seq None) or the table [V,H] with ids seq [B,T]; inputs already validated.
    The extractor states hs are a differentiable output: a gradient that reaches them (the
    auxiliary loss's) enters the extractor's chain through rk_dien_interest_backward_aux; none
    (hs unused) is a null pointer there, and the call is rk_dien_interest_backward's."""

    @staticmethod
    def forward(ctx, query, keys, seq, keys_length, cell, nh, *ws):
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None, not as zeros
        dense = seq is None
        B, H = query.shape
        T = keys.shape[1] if dense else seq.shape[1]
        dev = query.device
        f32 = dict(device=dev, dtype=torch.float32)
        ws = [w.contiguous() for w in ws]
        out, att = torch.empty(B, nh, **f32), torch.empty(B, T, **f32)
        hs, ss = torch.empty(B, T, nh, **f32), torch.empty(B, T, nh, **f32)
        if B > 0:
            try:
                if dense:
                    ops.dien_interest_train_dense(query, keys, keys_length, nh, cell, ws, out, att, hs, ss)
                else:
                    ops.dien_interest_train(query.data_ptr(), query.stride(0), keys, seq, keys_length, T, H, nh, cell,
                                            ws, out.data_ptr(), out.stride(0), att, hs, ss, B, dev)
            except ops._lib.RankOpsError as e:
                _convert(e, H, nh, T)
        ctx.save_for_backward(query, keys, keys_length, att, hs, ss, *ws)
        ctx.seq, ctx.cell, ctx.nh = seq, cell, nh
        ctx.mark_non_differentiable(att)
        return out, att, hs

    @staticmethod
    def backward(ctx, d_out, _d_att, d_hs):
        query, keys, keys_length, att, hs, ss, *ws = ctx.saved_tensors
        seq, cell, nh = ctx.seq, ctx.cell, ctx.nh
        dense = seq is None
        B, H = query.shape
        T = keys.shape[1] if dense else seq.shape[1]
        dev = query.device
        f32 = dict(device=dev, dtype=torch.float32)
        if B == 0:
            return (torch.zeros_like(query), torch.zeros_like(keys), None, None, None, None,
                    *[torch.zeros_like(w) for w in ws])
        if d_out is None:  # only the states were used
            d_out = torch.zeros(B, nh, **f32)
        d_out = d_out.to(torch.float32)
        if d_out.stride(1) != 1 or d_out.stride(0) < nh:
            d_out = d_out.contiguous()
        if d_hs is not None:
            d_hs = d_hs.to(torch.float32).contiguous()
        dq = torch.empty(B, H, **f32)
        dkeys = torch.empty(B, T, H, **f32)
        ids = None if dense else torch.empty_like(seq)
        wgrads = ops.dien_interest_backward(query.data_ptr(), query.stride(0), keys, seq, keys.stride(0) if dense else 0,
                                            keys_length, T, H, nh, cell, ws, hs, ss, att, d_out.data_ptr(),
                                            d_out.stride(0), dq.data_ptr(), H, False, dkeys, B, dev, ids, d_hs=d_hs)
        if dense:
            dk = dkeys
        elif ctx.needs_input_grad[1]:
            dk = train.zero_grads([keys], dev)[0]
            ops.embedding_backward([ops.table_segment(dk, ids.reshape(-1), 0)], B * T, dkeys.view(B * T, H))
        else:
            dk = None
        return (dq, dk, None, None, None, None, *wgrads)


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _pack(out, att, hs, return_attention, return_states):
    if not (return_attention or return_states):
        return out
    return (out,) + ((att,) if return_attention else ()) + ((hs,) if return_states else ())


def dien_interest(query, keys, keys_length, weights, cell_type="AGRU", return_attention=False, return_states=False):
    """dien_interest(query[B,H], keys[B,T,H], keys_length[B], weights) -> final interest state [B,nh]
    (dien.py:198-229) on rk_dien_interest_dense: TF GRUCell over the keys, attention of the hidden
    states against `A . query` (softmax over all T positions, positions t >= keys_length masked
    with -2^32+1), then the AGRU / AUGRU cell over the hidden states for t < keys_length.
    `weights` = (Wg, bg, Wc, bc, A, Vg, vg, Vc, vc) device tensors (rankops.h);
    `return_attention` adds the attention weights [B,T], `return_states` (after them) the extractor
    states hs [B,T,nh] with rows t >= keys_length zero, what dien_aux_loss takes.  Differentiable
    w.r.t. query, keys and the weights (the attention output is not; hs is): with grad mode on and
    any of them requiring grad the call goes through rk_dien_interest_train_dense /
    rk_dien_interest_backward(_aux).  Without grad, return_states runs the train forward kernel."""
    cell = _cell(cell_type)
    query = ops.as_f32(query, "query")
    keys = ops.as_f32(keys, "keys")
    keys_length = ops.as_index(keys_length, "keys_length")
    if keys.dim() != 3 or query.dim() != 2 or query.shape[0] != keys.shape[0] or query.shape[1] != keys.shape[2]:
        raise ValueError(f"dien_interest: query {tuple(query.shape)} and keys {tuple(keys.shape)} do not match")
    B, T, H = keys.shape
    if keys_length.dim() != 1 or keys_length.shape[0] != B:
        raise ValueError(f"dien_interest: keys_length must be [{B}], got {tuple(keys_length.shape)}")
    ws, nh = _weights(weights, H)
    _check_envelope(H, nh, T)
    if keys.stride(2) != 1 or keys.stride(1) % 4 or keys.stride(0) % 4 or keys.data_ptr() % 16:
        keys = keys.contiguous()
    if query.stride(1) != 1:
        query = query.contiguous()
    if _wants_grad(query, keys, *weights):
        out, att, hs = _DIENInterest.apply(query, keys, None, keys_length.contiguous(), cell, nh, *ws)
        return _pack(out, att, hs, return_attention, return_states)
    f32 = dict(device=keys.device, dtype=torch.float32)
    out = torch.empty(B, nh, **f32)
    att = torch.empty(B, T, **f32) if return_attention or return_states else None
    hs = torch.empty(B, T, nh, **f32) if return_states else None
    if B > 0:
        try:
            if return_states:
                ops.dien_interest_train_dense(query, keys, keys_length.contiguous(), nh, cell, ws, out, att, hs,
                                              torch.empty(B, T, nh, **f32))
            else:
                ops.dien_interest_dense(query, keys, keys_length.contiguous(), nh, cell, ws, out, att)
        except ops._lib.RankOpsError as e:
            _convert(e, H, nh, T)
    return _pack(out, att, hs, return_attention, return_states)


def dien_interest_gather(query, table, seq, keys_length, weights, cell_type="AGRU", return_attention=False,
                         return_states=False):
    """dien_interest with the history given as (embedding table [V,H], ids [B,T]): the gather
    happens inside the kernel (rk_dien_interest); ids at t >= keys_length are never read.
    Differentiable like dien_interest; the table's gradient is dense (nn.Embedding's)."""
    cell = _cell(cell_type)
    query = ops.as_f32(query, "query")
    table = ops.as_f32(table, "table")
    seq = ops.as_index(seq, "keys index")
    keys_length = ops.as_index(keys_length, "keys_length")
    if query.dim() != 2 or table.dim() != 2 or seq.dim() != 2 or table.shape[1] != query.shape[1] \
            or seq.shape[0] != query.shape[0]:
        raise ValueError(f"dien_interest_gather: query {tuple(query.shape)}, table {tuple(table.shape)} and ids "
                         f"{tuple(seq.shape)} do not match")
    B, H = query.shape
    T = seq.shape[1]
    if keys_length.dim() != 1 or keys_length.shape[0] != B:
        raise ValueError(f"dien_interest_gather: keys_length must be [{B}], got {tuple(keys_length.shape)}")
    ws, nh = _weights(weights, H)
    _check_envelope(H, nh, T)
    if table.stride(1) != 1 or table.stride(0) % 4 or table.data_ptr() % 16:
        table = table.contiguous()
    if query.stride(1) != 1:
        query = query.contiguous()
    if _wants_grad(query, table, *weights):
        out, att, hs = _DIENInterest.apply(query, table, seq.contiguous(), keys_length.contiguous(), cell, nh, *ws)
        return _pack(out, att, hs, return_attention, return_states)
    f32 = dict(device=query.device, dtype=torch.float32)
    out = torch.empty(B, nh, **f32)
    att = torch.empty(B, T, **f32) if return_attention or return_states else None
    hs = torch.empty(B, T, nh, **f32) if return_states else None
    if B > 0:
        args = (query.data_ptr(), query.stride(0), table, seq.contiguous(), keys_length.contiguous(), T, H, nh, cell, ws,
                out.data_ptr(), out.stride(0), att)
        try:
            if return_states:
                ops.dien_interest_train(*args, hs, torch.empty(B, T, nh, **f32), B, query.device)
            else:
                ops.dien_interest(*args, B, query.device)
        except ops._lib.RankOpsError as e:
            _convert(e, H, nh, T)
    return _pack(out, att, hs, return_attention, return_states)


# ------------------------------------------------------------------ request-level scoring

def _extract_weights(weights, H: int):
    """The nine-tuple checked as dien_interest checks it; returns the extractor's four and nh."""
    ws, nh = _weights(weights, H)
    return ws[:4], nh


def dien_extract(keys, keys_length, weights):
    """dien_extract(keys[R,T,H], keys_length[R], weights) -> hs [R,T,nh]: the interest extractor (TF
    GRUCell over the history, pass 1 of dien_interest) once per request, on rk_dien_extract_dense.
    Rows t >= keys_length are zero; hs is bit-equal to dien_interest(..., return_states=True)'s.
    `weights` is dien_interest's nine-tuple, of which the first four (Wg, bg, Wc, bc) are used; hs
    is valid only for them.  Feed it to dien_evolve with one query per candidate.
    Inference only: the result carries no grad_fn; train through dien_interest."""
    keys = ops.as_f32(keys, "keys")
    keys_length = ops.as_index(keys_length, "keys_length")
    if keys.dim() != 3:
        raise ValueError(f"dien_extract: keys must be [R, T, H], got {tuple(keys.shape)}")
    R, T, H = keys.shape
    if keys_length.dim() != 1 or keys_length.shape[0] != R:
        raise ValueError(f"dien_extract: keys_length must be [{R}], got {tuple(keys_length.shape)}")
    ws, nh = _extract_weights(weights, H)
    _check_envelope(H, nh, T)
    keys = keys.detach()
    if keys.stride(2) != 1 or keys.stride(1) % 4 or keys.stride(0) % 4 or keys.data_ptr() % 16:
        keys = keys.contiguous()
    hs = torch.empty(R, T, nh, device=keys.device, dtype=torch.float32)
    if R > 0:
        try:
            ops.dien_extract_dense(keys, keys_length.contiguous(), nh, [w.detach() for w in ws], hs)
        except ops._lib.RankOpsError as e:
            _convert(e, H, nh, T)
    return hs


def dien_extract_gather(table, seq, keys_length, weights):
    """dien_extract with the histories given as (embedding table [V,H], ids [R,T]): the gather
    happens inside the kernel (rk_dien_extract); ids at t >= keys_length are never read.
    Bit-equal to dien_extract(table[seq], ...).
    Inference only: the result carries no grad_fn; train through dien_interest_gather."""
    table = ops.as_f32(table, "table")
    seq = ops.as_index(seq, "keys index")
    keys_length = ops.as_index(keys_length, "keys_length")
    if table.dim() != 2 or seq.dim() != 2:
        raise ValueError(f"dien_extract_gather: table {tuple(table.shape)} and ids {tuple(seq.shape)} do not match")
    R, T = seq.shape
    H = table.shape[1]
    if keys_length.dim() != 1 or keys_length.shape[0] != R:
        raise ValueError(f"dien_extract_gather: keys_length must be [{R}], got {tuple(keys_length.shape)}")
    ws, nh = _extract_weights(weights, H)
    _check_envelope(H, nh, T)
    table = table.detach()
    if table.stride(1) != 1 or table.stride(0) % 4 or table.data_ptr() % 16:
        table = table.contiguous()
    hs = torch.empty(R, T, nh, device=table.device, dtype=torch.float32)
    if R > 0:
        try:
            ops.dien_extract(table, seq.contiguous(), keys_length.contiguous(), T, H, nh, [w.detach() for w in ws],
                             hs, R, table.device)
        except ops._lib.RankOpsError as e:
            _convert(e, H, nh, T)
    return hs


def dien_evolve(query, hs, keys_length, request_index, weights, cell_type="AGRU", return_attention=False):
    """dien_evolve(query[B,H], hs[R,T,nh], keys_length[R], request_index[B], weights) -> final interest
    state [B,nh] on rk_dien_evolve: candidate b is scored against the history of request
    request_index[b] (any order; a request may have no candidate or many): attention of hs against
    `A . query`, masked softmax over all T positions, then the AGRU / AUGRU cell over hs for
    t < keys_length.  `return_attention` adds the attention weights [B,T].  State and attention
    are bit-equal to dien_interest with that request's history repeated for every candidate.
    `weights` is dien_interest's nine-tuple, of which the last five (A, Vg, vg, Vc, vc) are used;
    `hs` and `keys_length` are dien_extract's, computed with the same nine.  Rows of hs at
    t >= keys_length are never read; a request_index outside [0, R) gives a zero state and raises
    the index-out-of-range flag (rankops.error_flags()).
    Inference only: the results carry no grad_fn; train through dien_interest."""
    cell = _cell(cell_type)
    query = ops.as_f32(query, "query")
    hs = ops.as_f32(hs, "hs")
    keys_length = ops.as_index(keys_length, "keys_length")
    request_index = ops.as_index(request_index, "request_index")
    if query.dim() != 2 or hs.dim() != 3:
        raise ValueError(f"dien_evolve: query {tuple(query.shape)} must be [B, H] and hs {tuple(hs.shape)} [R, T, nh]")
    B, H = query.shape
    R, T, _ = hs.shape
    if keys_length.dim() != 1 or keys_length.shape[0] != R:
        raise ValueError(f"dien_evolve: keys_length must be [{R}], got {tuple(keys_length.shape)}")
    if request_index.dim() != 1 or request_index.shape[0] != B:
        raise ValueError(f"dien_evolve: request_index must be [{B}], one request per query row, got "
                         f"{tuple(request_index.shape)}")
    ws, nh = _weights(weights, H)
    if hs.shape[2] != nh:
        raise ValueError(f"dien_evolve: hs must be [R, T, {nh}], got {tuple(hs.shape)}")
    _check_envelope(H, nh, T)
    if B > 0 and R == 0:
        raise ValueError("dien_evolve: hs holds no request, yet request_index names one per query row")
    query, hs = query.detach(), hs.detach().contiguous()
    if query.stride(1) != 1:
        query = query.contiguous()
    f32 = dict(device=query.device, dtype=torch.float32)
    out = torch.empty(B, nh, **f32)
    att = torch.empty(B, T, **f32) if return_attention else None
    if B > 0:
        try:
            ops.dien_evolve(query.data_ptr(), query.stride(0), hs, keys_length.contiguous(), request_index.contiguous(),
                            H, cell, [w.detach() for w in ws[4:]], out.data_ptr(), out.stride(0), att, B, query.device)
        except ops._lib.RankOpsError as e:
            _convert(e, H, nh, T)
    return (out, att) if return_attention else out


class DIENInterests:
    """What DIEN.extract_interests returns: `hs` [R, T, nh], the extractor states of R behaviour
    histories, and `keys_length` [R].  Valid only for the weights it was computed with: a cache
    of these keyed by user must be dropped after every weight update."""
    __slots__ = ("hs", "keys_length")

    def __init__(self, hs, keys_length):
        self.hs = hs
        self.keys_length = keys_length

    def __len__(self):
        return self.hs.shape[0]


AUX_ENVELOPE = ENVELOPE + f", 1 <= T_neg (negatives per step) <= {ops.DIEN_AUX_MAX_NEG}"


def _convert_aux(rc_error, H, nh, T, T_neg):
    if getattr(rc_error, "code", None) == ops._lib.RK_ERR_UNSUPPORTED:
        raise NotImplementedError(f"rankops dien_aux_loss: H={H}, nh={nh}, T={T}, T_neg={T_neg}: {rc_error}; "
                                  f"envelope: {AUX_ENVELOPE}") from rc_error
    raise rc_error


def _negatives_per_step(count: int, T: int, what: str) -> int:
    """T_neg from the negatives' second dimension, (T-1) * T_neg entries (entry t * T_neg + n pairs with h_t)."""
    if T == 1:
        if count != 0:
            raise ValueError(f"{what}: T = 1 leaves no step to supervise, the negatives must be empty, got {count}")
        return 1
    if count == 0 or count % (T - 1) != 0:
        raise ValueError(f"{what}: the negatives' second dimension must be a positive multiple of T-1 = {T - 1} "
                         f"(T_neg per step), got {count}")
    return count // (T - 1)


def _check_aux_envelope(H: int, nh: int, T: int, T_neg: int):
    if H not in (8, 16, 32) or nh not in (8, 16) or not 1 <= T <= 256 or not 1 <= T_neg <= ops.DIEN_AUX_MAX_NEG:
        raise NotImplementedError(f"rankops dien_aux_loss: H={H}, nh={nh}, T={T}, T_neg={T_neg} is outside the "
                                  f"kernel's envelope: {AUX_ENVELOPE}")


class _DIENAuxLoss(torch.autograd.Function):
    """dien_aux_loss / dien_aux_loss_gather under autograd: rk_dien_aux_loss(_dense) forward,
    rk_dien_aux_loss_backward (which recomputes the dots and reads the upstream scalar from device
    memory).  `keys` is the history [B,T,H] with `neg` [B,(T-1)T_neg,H] (seq None), or the table
    [V,H] with ids seq [B,T] and neg_seq [B,(T-1)T_neg] (neg None); inputs already validated.
    Returns (mean loss, per-sample loss); only the mean is differentiable."""

    @staticmethod
    def forward(ctx, hs, keys, neg, w_aux, seq, neg_seq, keys_length, T_neg):
        dense = seq is None
        B, T, nh = hs.shape
        H = w_aux.shape[0]
        dev = hs.device
        per_sample = torch.empty(B, device=dev, dtype=torch.float32)
        mean = torch.empty(1, device=dev, dtype=torch.float32)
        try:
            ops.dien_aux_loss(hs, keys, seq, neg, neg_seq, keys_length, T, T_neg, H, nh, w_aux, per_sample, mean, B,
                              dev)
        except ops._lib.RankOpsError as e:
            _convert_aux(e, H, nh, T, T_neg)
        ctx.save_for_backward(hs, keys, w_aux, keys_length, *([neg] if dense else []))
        ctx.seq, ctx.neg_seq, ctx.T_neg = seq, neg_seq, T_neg
        ctx.mark_non_differentiable(per_sample)
        return mean.reshape(()), per_sample

    @staticmethod
    def backward(ctx, d_mean, _d_per_sample):
        hs, keys, w_aux, keys_length, *rest = ctx.saved_tensors
        seq, neg_seq, T_neg = ctx.seq, ctx.neg_seq, ctx.T_neg
        dense = seq is None
        neg = rest[0] if dense else None
        B, T, nh = hs.shape
        H = w_aux.shape[0]
        dev = hs.device
        if B == 0:
            return (torch.zeros_like(hs), torch.zeros_like(keys), None if neg is None else torch.zeros_like(neg),
                    torch.zeros_like(w_aux), None, None, None, None)
        d_loss = d_mean.to(torch.float32).reshape(1).contiguous()
        ids = None if dense else torch.empty_like(seq)
        neg_ids = None if dense else torch.empty_like(neg_seq)
        d_hs, dkeys, dneg, dw = ops.dien_aux_loss_backward(hs, keys, seq, neg, neg_seq, keys_length, T, T_neg, H, nh,
                                                           w_aux, d_loss, B, dev, ids, neg_ids)
        if dense:
            return d_hs, dkeys, dneg, dw, None, None, None, None
        dk = None
        if ctx.needs_input_grad[1]:  # the dense table gradient: positives and negatives into one buffer
            dk = train.zero_grads([keys], dev)[0]
            ops.embedding_backward([ops.table_segment(dk, ids.reshape(-1), 0)], B * T, dkeys.view(B * T, H))
            if T > 1:
                n = neg_ids.numel()
                ops.embedding_backward([ops.table_segment(dk, neg_ids.reshape(-1), 0)], n, dneg.view(n, H))
        return d_hs, dk, None, dw, None, None, None, None


def _aux_common(hs, keys_length, w_aux, B, T, H, what):
    hs = ops.as_f32(hs, "hs")
    w_aux = ops.as_f32(w_aux, "w_aux")
    keys_length = ops.as_index(keys_length, "keys_length")
    if w_aux.dim() != 2 or w_aux.shape[0] != H:
        raise ValueError(f"{what}: w_aux must be [{H}, nh], got {tuple(w_aux.shape)}")
    nh = w_aux.shape[1]
    if tuple(hs.shape) != (B, T, nh):
        raise ValueError(f"{what}: hs must be [{B}, {T}, {nh}], got {tuple(hs.shape)}")
    if keys_length.dim() != 1 or keys_length.shape[0] != B:
        raise ValueError(f"{what}: keys_length must be [{B}], got {tuple(keys_length.shape)}")
    return hs.contiguous(), keys_length.contiguous(), w_aux.contiguous(), nh


def dien_aux_loss(hs, keys, neg_keys, keys_length, w_aux, return_per_sample=False):
    """DIEN's auxiliary loss (dien.py:256-300 with the paper's sign) on rk_dien_aux_loss_dense:
    hs [B,T,nh] the extractor states (dien_interest(..., return_states=True)), keys [B,T,H] the
    history, neg_keys [B,(T-1)*T_neg,H] the sampled negatives (entry t*T_neg+n pairs with h_t; T_neg
    is inferred), w_aux [H,nh].  With g_t = w_aux h_t, per sample
    -sum_{t < len-1} [logsig(g_t . keys[t+1]) + sum_n logsig(-(g_t . neg[t,n]))]; returns the batch mean
    (a 0-dim tensor), with `return_per_sample` also the [B] per-sample values (not differentiable).
    Differentiable w.r.t. hs, keys, neg_keys and w_aux."""
    what = "dien_aux_loss"
    keys = ops.as_f32(keys, "keys")
    neg_keys = ops.as_f32(neg_keys, "neg_keys")
    if keys.dim() != 3 or neg_keys.dim() != 3 or neg_keys.shape[0] != keys.shape[0] or neg_keys.shape[2] != keys.shape[2]:
        raise ValueError(f"{what}: keys {tuple(keys.shape)} and neg_keys {tuple(neg_keys.shape)} do not match")
    B, T, H = keys.shape
    hs, keys_length, w_aux, nh = _aux_common(hs, keys_length, w_aux, B, T, H, what)
    T_neg = _negatives_per_step(neg_keys.shape[1], T, what)
    _check_aux_envelope(H, nh, T, T_neg)
    if keys.stride(2) != 1 or keys.stride(1) % 4 or keys.stride(0) % 4 or keys.data_ptr() % 16:
        keys = keys.contiguous()
    if neg_keys.stride(2) != 1 or neg_keys.stride(1) % 4 or neg_keys.stride(0) % 4 or neg_keys.data_ptr() % 16:
        neg_keys = neg_keys.contiguous()
    mean, per_sample = _DIENAuxLoss.apply(hs, keys, neg_keys, w_aux, None, None, keys_length, T_neg)
    return (mean, per_sample) if return_per_sample else mean


def dien_aux_loss_gather(hs, table, seq, neg_seq, keys_length, w_aux, return_per_sample=False):
    """dien_aux_loss with the history and the negatives given as ids into one embedding table [V,H]:
    seq [B,T], neg_seq [B,(T-1)*T_neg]; the gathers happen inside the kernel (rk_dien_aux_loss), ids
    of masked steps are never read.  The table's gradient is dense (nn.Embedding's) and takes the
    positives' and the negatives' rows."""
    what = "dien_aux_loss_gather"
    table = ops.as_f32(table, "table")
    seq = ops.as_index(seq, "keys index")
    neg_seq = ops.as_index(neg_seq, "negatives index")
    if table.dim() != 2 or seq.dim() != 2 or neg_seq.dim() != 2 or neg_seq.shape[0] != seq.shape[0]:
        raise ValueError(f"{what}: table {tuple(table.shape)}, ids {tuple(seq.shape)} and negative ids "
                         f"{tuple(neg_seq.shape)} do not match")
    B, T = seq.shape
    H = table.shape[1]
    hs, keys_length, w_aux, nh = _aux_common(hs, keys_length, w_aux, B, T, H, what)
    T_neg = _negatives_per_step(neg_seq.shape[1], T, what)
    _check_aux_envelope(H, nh, T, T_neg)
    if table.stride(1) != 1 or table.stride(0) % 4 or table.data_ptr() % 16:
        table = table.contiguous()
    mean, per_sample = _DIENAuxLoss.apply(hs, table, None, w_aux, seq.contiguous(), neg_seq.contiguous(), keys_length,
                                          T_neg)
    return (mean, per_sample) if return_per_sample else mean


def _tf_linear(in_features: int, out_features: int, bias_value: float = 0.0) -> nn.Linear:
    """nn.Linear initialised as a TF dense / _Linear layer: Glorot-uniform kernel, constant bias."""
    lin = nn.Linear(in_features, out_features)
    nn.init.xavier_uniform_(lin.weight)
    nn.init.constant_(lin.bias, bias_value)
    return lin


class DIEN(EngineModule):
    def __init__(self, vocab_dir, hidden_units=None, activation='dice', dropout_rate=0.1, batch_norm=True,
                 custom_gru_type='AGRU', gru_output_units=8, *, vocab_sizes=None, embedding_dim=16,
                 trainable=False, use_auxiliary_loss=False, negative_sample_number=3, sparse_grad=False):
        super().__init__()
        self.sparse_grad = bool(sparse_grad)  # train mode: tables get sparse COO gradients (rankops.SparseAdam)
        self.use_auxiliary_loss = bool(use_auxiliary_loss)
        self.negative_sample_number = int(negative_sample_number)
        if self.use_auxiliary_loss and self.negative_sample_number < 1:
            raise ValueError(f"rankops DIEN: negative_sample_number must be >= 1, got {negative_sample_number}")
        self.trainable = bool(trainable)  # train mode is opt-in; parameters and initialisation are the same
        self._dropout = train.DropoutStreams()
        if hidden_units is None:
            hidden_units = [512, 256, 128]
        _cell(custom_gru_type)
        self.activation = activation
        self.dropout_rate = dropout_rate
        self.batch_norm = batch_norm
        self.custom_gru_type = custom_gru_type
        self.gru_output_units = nh = gru_output_units
        self.vocab_sizes = {f: table_rows(vocab_dir, f, vocab_sizes) for f in FIELDS}
        self.num_dense_features = 16
        # target and history share the feedid table (shared_embedding_columns, dien.py:126)
        self.embeddings = nn.ModuleDict({
            "userid": nn.Embedding(self.vocab_sizes["userid"], 16),
            "device": nn.Embedding(self.vocab_sizes["device"], 2),
            "authorid": nn.Embedding(self.vocab_sizes["authorid"], 4),
            "bgm_song_id": nn.Embedding(self.vocab_sizes["bgm_song_id"], 4),
            "bgm_singer_id": nn.Embedding(self.vocab_sizes["bgm_singer_id"], 4),
            "manual_tag_list": nn.Embedding(self.vocab_sizes["manual_tag_list"], 4),
            "feedid": nn.Embedding(self.vocab_sizes["feedid"], embedding_dim),
        })
        H = embedding_dim
        self.gru = nn.ModuleDict({"gates": _tf_linear(H + nh, 2 * nh, 1.0), "candidate": _tf_linear(H + nh, nh)})
        self.attention_project_matrix = nn.Parameter(nn.init.xavier_uniform_(torch.empty(nh, H)))
        self.evolution = nn.ModuleDict({"gates": _tf_linear(2 * nh, 2 * nh, 1.0),
                                        "candidate": _tf_linear(2 * nh, nh)})
        width = self.num_dense_features + H + nh
        for key in ("userid", "device", "authorid", "bgm_song_id", "bgm_singer_id", "manual_tag_list"):
            width += self.embeddings[key].embedding_dim
        self.fcn = nn.ModuleList()
        self._tail = []
        for unit in hidden_units:
            lin = _tf_linear(width, unit)
            self.fcn.append(lin)
            if activation == 'dice':
                act, kind = Dice(unit), "dice"
            else:
                act, kind = nn.PReLU(), "prelu"
            self.fcn.append(act)
            bn = None
            if batch_norm:
                bn = nn.BatchNorm1d(unit)
                self.fcn.append(bn)
            if dropout_rate > 0:
                self.fcn.append(nn.Dropout(dropout_rate))
            self._tail.append(Layer(lin, act=kind, act_module=act, post_bn=bn))
            width = unit
        self.output_layer = _tf_linear(width, 1)
        # last, and only with the flag: a default model's parameters, their order and the random
        # numbers their initialisation draws are untouched (aux_project_matrix, dien.py:268)
        if self.use_auxiliary_loss:
            self.aux_project_matrix = nn.Parameter(nn.init.xavier_uniform_(torch.empty(H, nh)))

    def _aux_active(self) -> bool:
        return self.use_auxiliary_loss and self.training

    def _load_vocabulary(self, vocab_dir, filename):
        return load_vocabulary(vocab_dir, filename)

    def interest_weights(self):
        """(Wg, bg, Wc, bc, A, Vg, vg, Vc, vc) as dien_interest takes them."""
        return (self.gru["gates"].weight, self.gru["gates"].bias, self.gru["candidate"].weight,
                self.gru["candidate"].bias, self.attention_project_matrix, self.evolution["gates"].weight,
                self.evolution["gates"].bias, self.evolution["candidate"].weight, self.evolution["candidate"].bias)

    @staticmethod
    def _history(sequence):
        """(ids [B, T], lengths [B]) of the behaviour history, contiguous int64."""
        seq = ops.as_index(sequence[SEQ_KEY], f"sequence[{SEQ_KEY!r}]").contiguous()
        seq_len = ops.as_index(sequence[f"{SEQ_KEY}_length"], "sequence length").contiguous()
        return seq, seq_len

    def _plan(self, dense, category, sequence, target):
        """Row layout [dense | category | target | final interest state] and the gather segments
        (dien.py:179-191,237)."""
        dense_cols = [ops.as_f32(v, f"dense[{k!r}]") for k, v in dense.items()]
        B = dense_cols[0].shape[0]
        dev = dense_cols[0].device
        segs = [ops.dense_segment(v, 1, i) for i, v in enumerate(dense_cols)]
        col = len(dense_cols)
        lookups = []  # (table weight, index, column) for the training backward
        for name, emb in self.embeddings.items():
            if name != "feedid" and name in category:
                idx = ops.as_index(category[name], f"category[{name!r}]")
                segs.append(ops.table_segment(emb.weight, idx, col))
                lookups.append((emb.weight, idx, col))
                col += emb.embedding_dim
        tgt = self.embeddings["feedid"]
        tgt_idx = ops.as_index(target["feedid"], "target['feedid']")
        segs.append(ops.table_segment(tgt.weight, tgt_idx, col))
        lookups.append((tgt.weight, tgt_idx, col))
        q_col = col
        state_col = q_col + tgt.embedding_dim
        seq, seq_len = (None, None) if sequence is None else self._history(sequence)  # None: score()
        return dict(B=B, dev=dev, segs=segs, lookups=lookups, q_col=q_col, state_col=state_col,
                    width=state_col + self.gru_output_units, H=tgt.embedding_dim, seq=seq, seq_len=seq_len)

    def forward(self, dense, category, sequence, target, return_attention=False):
        if not self.trainable:
            check_eval(self)
        tgt = target.get("feedid", None) if isinstance(target, dict) else None
        if isinstance(tgt, torch.Tensor) and tgt.shape[0] == 0:  # an empty batch: nothing to launch
            dev = ops.require_gpu(tgt, "target['feedid']").device
            out = common.empty_rows(dev, 2)
            return out + (torch.zeros((), device=dev),) if self._aux_active() else out
        pl = self._plan(dense, category, sequence, target)
        B, dev, H, nh, width = pl["B"], pl["dev"], pl["H"], self.gru_output_units, pl["width"]
        if width != self._tail[0].linear.in_features:
            raise ValueError(f"rankops DIEN: the inputs make a row of {width} columns, the first fcn layer takes "
                             f"{self._tail[0].linear.in_features}")
        T = pl["seq"].shape[1]
        _check_envelope(H, nh, T)
        if self._aux_active():  # the negatives of the auxiliary loss: ids into the feedid table
            T_neg = self.negative_sample_number
            if NEG_SEQ_KEY not in sequence:
                raise ValueError(f"rankops DIEN: use_auxiliary_loss=True needs sequence[{NEG_SEQ_KEY!r}], the sampled "
                                 f"negatives [B, (T-1)*negative_sample_number] (entry t*T_neg+n pairs with step t)")
            neg = ops.as_index(sequence[NEG_SEQ_KEY], f"sequence[{NEG_SEQ_KEY!r}]")
            if tuple(neg.shape) != (B, (T - 1) * T_neg):
                raise ValueError(f"rankops DIEN: sequence[{NEG_SEQ_KEY!r}] must be [B, (T-1)*negative_sample_number] = "
                                 f"[{B}, {(T - 1) * T_neg}], got {tuple(neg.shape)}")
            _check_aux_envelope(H, nh, T, T_neg)
            pl["neg_seq"] = neg.contiguous()
        if self.training:  # Dice / BatchNorm batch statistics, Dropout, HIP backward (rankops.train)
            grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
            try:
                prob, logit, att, *aux = train.dien_train_forward(self, pl, grad)
            except ops._lib.RankOpsError as e:
                _convert(e, H, nh, T)
            return (prob, logit, att, *aux) if return_attention else (prob, logit, *aux)
        logit = torch.empty(B, 1, device=dev, dtype=torch.float32)
        prob = torch.empty(B, 1, device=dev, dtype=torch.float32)
        att = torch.empty(B, T, device=dev, dtype=torch.float32) if return_attention else None
        if self._fusable(pl, T):
            # the whole forward in one launch (rk_dien_forward); outside its envelope the three below,
            # which compute the same bits
            try:
                self._launch_fused(pl, logit, prob, att)
                return (prob, logit, att) if return_attention else (prob, logit)
            except ops._lib.RankOpsError as e:
                if getattr(e, "code", None) != ops._lib.RK_ERR_UNSUPPORTED:
                    raise
                self._mark_unfusable(pl, T)
        row = torch.empty(B, width, device=dev, dtype=torch.float32)
        ops.concat_gather(pl["segs"], B, row)
        try:
            ops.dien_interest(ops._lib.fptr(row, pl["q_col"]), width, self.embeddings["feedid"].weight, pl["seq"],
                              pl["seq_len"], T, H, nh, _cell(self.custom_gru_type), self.interest_weights(),
                              ops._lib.fptr(row, pl["state_col"]), width, att, B, dev)
        except ops._lib.RankOpsError as e:
            _convert(e, H, nh, T)
        run_tail(row, self._tail, self.output_layer, {}, logit, prob)
        return (prob, logit, att) if return_attention else (prob, logit)

    # ---- the one-launch forward (rk_dien_forward) and its prepared form

    def _fusable(self, pl, T) -> bool:
        """Whether the eval forward tries rk_dien_forward: the switch, the cheap half of its envelope
        (the library checks all of it and answers RK_ERR_UNSUPPORTED), no earlier refusal of the
        shape, and a batch that gives no CU a second workgroup (a workgroup holds 4 chain waves among
        its 16 and a CU holds one workgroup, so past that the recurrence of rk_dien_interest's one-wave
        workgroups, many per CU, is faster than the launches saved).  It needs run_tail's fused path
        for the bits to be the three launches'."""
        per_cu = common.FUSED_DIEN_WG_PER_CU
        return (common.FUSED_DIEN and common.FUSED_MLP and self.gru_output_units == 8 and pl["H"] in (8, 16, 32)
                and fused_mlp_fits(pl["width"], [l.linear.out_features for l in self._tail])
                and (per_cu is None or (pl["B"] + 15) // 16 <= per_cu * common._num_cus(pl["dev"]))
                and (pl["width"], T, pl["H"]) not in self.__dict__.get("_unfusable", ()))

    def _mark_unfusable(self, pl, T):
        """rk_dien_forward refused this shape (RK_ERR_UNSUPPORTED, e.g. its LDS need at a long history):
        later forwards of the shape take the three launches at once."""
        self.__dict__.setdefault("_unfusable", set()).add((pl["width"], T, pl["H"]))

    def _fused_args(self, pl, packed, logit, prob, att):
        layers = [ops.make_mlp_layer(l.linear.weight, pk, **l.epilogue_kwargs()) for l, pk in zip(self._tail, packed)]
        head = ops.make_epilogue(head_w=self.output_layer.weight, head_b=self.output_layer.bias,
                                 head_logit=logit, head_prob=prob)
        return (pl["segs"], pl["width"], pl["q_col"], pl["state_col"], self.embeddings["feedid"].weight, pl["seq"],
                pl["seq_len"], pl["H"], self.gru_output_units, _cell(self.custom_gru_type), self.interest_weights(),
                layers, head, att, pl["B"], pl["dev"])

    def _launch_fused(self, pl, logit, prob, att):
        ops.dien_forward(*self._fused_args(pl, [PACKED(l.linear.weight) for l in self._tail], logit, prob, att))

    def prepare(self, dense, category, sequence, target):
        """An eval forward bound to these input tensors (the single-kernel analogue of capturing
        the forward in a hipGraph): returns `run()` that recomputes the whole forward from the
        current contents of the inputs with one kernel launch (rk_dien_forward_plan /
        rk_dien_plan_launch) and returns the same (prob, logit) tensors each time; `run.plan` is the
        plan.  The binding is by address: an input that would need a converted copy (not float32 /
        int64, a history that is not contiguous) raises instead of being bound to a copy.  Unlike
        `forward` it takes the one launch at any batch: past one 16-sample workgroup per CU a
        hipGraph of the three launches is faster.  Like a captured graph it binds the current
        weights: prepare again after changing them."""
        if self.training:
            raise RuntimeError("DIEN.prepare: eval mode only (call .eval() first)")
        pl = self._plan(dense, category, sequence, target)
        B, dev, width = pl["B"], pl["dev"], pl["width"]
        T = pl["seq"].shape[1]
        ids = [v for k, v in category.items() if k != "feedid" and k in self.embeddings]
        ids += [target["feedid"], sequence[SEQ_KEY], sequence[f"{SEQ_KEY}_length"]]
        if any(t.dtype != torch.int64 for t in ids) or any(v.dtype != torch.float32 for v in dense.values()) \
                or not all(t.is_contiguous() for t in ids[-2:]):
            raise RuntimeError("DIEN.prepare: the inputs must be the caller's own float32 / int64 tensors (the history "
                               "contiguous): a converted copy would stop following later writes")
        if B == 0:
            raise RuntimeError("DIEN.prepare: an empty batch has nothing to launch")
        if width != self._tail[0].linear.in_features:
            raise ValueError(f"rankops DIEN: the inputs make a row of {width} columns, the first fcn layer takes "
                             f"{self._tail[0].linear.in_features}")
        if not (common.FUSED_MLP and self.gru_output_units == 8 and pl["H"] in (8, 16, 32)
                and fused_mlp_fits(width, [l.linear.out_features for l in self._tail])):
            raise RuntimeError("DIEN.prepare: configuration outside rk_dien_forward's envelope")
        logit = torch.empty(B, 1, device=dev, dtype=torch.float32)
        prob = torch.empty(B, 1, device=dev, dtype=torch.float32)
        packed = [PACKED.pin(l.linear.weight) for l in self._tail]  # never rewritten under the plan
        args = self._fused_args(pl, packed, logit, prob, None)
        keep = (pl, packed, [l.epilogue_kwargs() for l in self._tail], args[10], args[11], logit, prob,
                self.embeddings["feedid"].weight, self.output_layer.weight, self.output_layer.bias)
        try:
            plan = ops.dien_forward_plan(*args, keep=keep)
        except ops._lib.RankOpsError as e:
            if getattr(e, "code", None) != ops._lib.RK_ERR_UNSUPPORTED:
                raise
            raise RuntimeError(f"DIEN.prepare: configuration outside rk_dien_forward's envelope: {e}") from e
        out = (prob, logit)

        def run():
            plan.launch()
            return out
        run.plan = plan
        return run

    # ---- request-level scoring (eval only): one history per request, many candidates per history

    def extract_interests(self, sequence) -> DIENInterests:
        """The interest extractor over R behaviour histories, `sequence[SEQ_KEY]` [R, T] with its
        `_length` [R], on rk_dien_extract: what `forward` computes before it looks at the target.
        Returns a DIENInterests (hs [R, T, nh] and the lengths) for `score`.  It is valid only for
        the weights it was computed with (the feedid table and gru.*): a cache of these keyed by
        user must be dropped after a weight update.  Eval mode only, no grad_fn."""
        check_eval(self)
        seq, seq_len = self._history(sequence)
        if seq.dim() != 2 or seq_len.dim() != 1 or seq_len.shape[0] != seq.shape[0]:
            raise ValueError(f"rankops DIEN: the history must be ids [R, T] with lengths [R], got "
                             f"{tuple(seq.shape)} and {tuple(seq_len.shape)}")
        return DIENInterests(dien_extract_gather(self.embeddings["feedid"].weight, seq, seq_len,
                                                 self.interest_weights()), seq_len)

    def score(self, dense, category, target, interests, request_index, return_attention=False):
        """`forward` for B candidates of R requests whose interests were extracted once:
        `interests` is `extract_interests`' result, `request_index` [B] names each candidate's
        request (any order), dense / category / target are per candidate as in `forward`.
        Returns (probability, logit), plus the attention weights [B, T] on request: bit-equal to
        `forward` with each request's history repeated for its candidates.  Launches:
        rk_concat_gather, rk_dien_evolve into the row's state columns, the fcn tail.  Eval mode
        only, no grad_fn."""
        check_eval(self)
        if not isinstance(interests, DIENInterests):
            raise TypeError(f"rankops DIEN: interests must be what extract_interests returns, got "
                            f"{type(interests).__name__}")
        request_index = ops.as_index(request_index, "request_index")
        if request_index.dim() != 1:
            raise ValueError(f"rankops DIEN: request_index must be [B], got {tuple(request_index.shape)}")
        hs = ops.as_f32(interests.hs, "interests.hs")
        lens = ops.as_index(interests.keys_length, "interests.keys_length")
        if hs.dim() != 3 or lens.dim() != 1 or lens.shape[0] != hs.shape[0]:
            raise ValueError(f"rankops DIEN: interests must hold hs [R, T, nh] and lengths [R], got "
                             f"{tuple(hs.shape)} and {tuple(lens.shape)}")
        R, T, nh = hs.shape
        dev = request_index.device
        if request_index.shape[0] == 0:  # no candidate: nothing to launch
            out = common.empty_rows(dev, 2)
            return out + (torch.empty(0, T, device=dev, dtype=torch.float32),) if return_attention else out
        pl = self._plan(dense, category, None, target)
        B, H, width = pl["B"], pl["H"], pl["width"]
        if request_index.shape[0] != B:
            raise ValueError(f"rankops DIEN: request_index must name one request for each of the {B} candidates, got "
                             f"{tuple(request_index.shape)}")
        if nh != self.gru_output_units:
            raise ValueError(f"rankops DIEN: interests of {nh} units, the model has {self.gru_output_units}")
        if R == 0:
            raise ValueError("rankops DIEN: interests holds no request, yet request_index names one per candidate")
        if width != self._tail[0].linear.in_features:
            raise ValueError(f"rankops DIEN: the inputs make a row of {width} columns, the first fcn layer takes "
                             f"{self._tail[0].linear.in_features}")
        _check_envelope(H, nh, T)
        logit = torch.empty(B, 1, device=dev, dtype=torch.float32)
        prob = torch.empty(B, 1, device=dev, dtype=torch.float32)
        row = torch.empty(B, width, device=dev, dtype=torch.float32)
        att = torch.empty(B, T, device=dev, dtype=torch.float32) if return_attention else None
        ops.concat_gather(pl["segs"], B, row)
        try:
            ops.dien_evolve(ops._lib.fptr(row, pl["q_col"]), width, hs.detach().contiguous(), lens.contiguous(),
                            request_index.contiguous(), H, _cell(self.custom_gru_type), self.interest_weights()[4:],
                            ops._lib.fptr(row, pl["state_col"]), width, att, B, dev)
        except ops._lib.RankOpsError as e:
            _convert(e, H, nh, T)
        run_tail(row, self._tail, self.output_layer, {}, logit, prob)
        return (prob, logit, att) if return_attention else (prob, logit)

    def rank(self, dense, category, target, interests, request_index, k):
        """`score`, then the best k candidates of each request: (RequestTopK, probability, logit),
        the top-K's indices being rows of the candidate batch.  Ranked on the logit: fp32
        probabilities saturate into ties where the logits still differ.  The request count is
        `interests`'; a request without candidates gets counts 0.  Eval mode only, as `score`."""
        from .ranking import topk_per_request
        prob, logit = self.score(dense, category, target, interests, request_index)
        top = topk_per_request(logit, ops.as_index(request_index, "request_index"), int(interests.hs.shape[0]), k)
        return top, prob, logit
