"""Training on the rankops engine.

The reference scripts train with autograd and torch.optim.Adam:

    model.train(); optimizer = optim.Adam(model.parameters(), lr=...)          # dcn.py:275
    optimizer.zero_grad(); prob, logit = model(dense, category)                # dcn.py:195-196
    loss = criterion(logit.squeeze(), label); loss.backward(); optimizer.step()  # dcn.py:198-201

A rankops model in train mode returns outputs attached to a `torch.autograd.Function` whose
forward runs the HIP forward kernels with the activations the backward needs kept in HBM, and
whose backward runs the HIP backward kernels (include/rankops.h, "training") and hands the
parameter gradients back to autograd — so `loss.backward()` fills every `.grad` as the
reference does and the unchanged loop works with `torch.optim.Adam` or with `rankops.Adam`
(the same update as one fused launch over all tensors, `rk_adam_step`).

Every model trains: DCNModel (`dcn.py:114-180`), DeepCrossingModel (`deepcrossing.py:106-163`)
and AFM (`afm.py:64-119`) — no BatchNorm / Dropout, train and eval forwards coincide —, DeepFM
(`deepfm.py:73-151`: BatchNorm batch statistics, Dropout), DIN (`din.py:225-323`: Dice and
BatchNorm batch statistics, Dropout, attention backward, l2 term), BSTModel (`bst.py:42-247`:
Dropout inside the transformer blocks, LayerNorm, attention backward) and FwFM (`fwfm.py:87-139`).
Dropout masks are a counter hash on the device (train_common.h): a random choice like torch's own
masks, so parity tests hand the engine's masks to the oracle.

Embedding gradients are dense by default (`nn.Embedding(sparse=False)`).  A model built with
`sparse_grad=True` hands every table a sparse COO gradient instead (`sparse_embedding_grads`), and
`rankops.SparseAdam` (`rk_sparse_adam_step`: torch.optim.SparseAdam / LazyAdam, `DIEN/dien.py:328`)
updates only the rows of the batch: the step then scales with the batch, not with the tables.
"""
from __future__ import annotations

import os

import torch
import torch.optim.optimizer as _optim_mod

from . import common, ops
from .common import PACKED, const, fused_mlp_fits


# BST blocks: the O / FFN2 projections and the residual LayerNorms after them as one launch each
# (rk_linear_res_dropout_ln) where the shape allows (d_model 128); False: two launches each.
FUSED_LN = os.environ.get("RANKOPS_FUSED_LN", "1") != "0"


# ---------------------------------------------------------------- shared pieces

def mlp_relu_forward(x, linears, head_w, head_b, partial, logit, prob):
    """Linear+ReLU stack with the Linear(N,1)+sigmoid head; returns the activations [x, h1, ...].
    The head reads head_partial (the other input block's share of the logit) when given."""
    B, dev = x.shape[0], x.device
    hs = [x] + [torch.empty(B, lin.out_features, device=dev, dtype=torch.float32) for lin in linears]
    if common.FUSED_MLP and fused_mlp_fits(x.shape[1], [lin.out_features for lin in linears]):
        # one rk_mlp_forward launch, each layer's activations also stored for the backward
        # under graph capture the packing is captured too (replays repack the updated weights);
        # a cached image would be frozen into the graph
        pack = ops.pack_mlp_weight if torch.cuda.is_current_stream_capturing() else PACKED
        # the packed images must stay referenced until the launch: the layer descriptors hold raw
        # pointers, and a freed image's block would be handed to the next allocation
        packed = [pack(lin.weight) for lin in linears]
        mls = [ops.make_mlp_layer(lin.weight, pw, bias=lin.bias, act="relu", store=y, ld_store=y.stride(0))
               for lin, pw, y in zip(linears, packed, hs[1:])]
        ep = ops.make_epilogue(head_w=head_w, head_b=head_b, head_logit=logit, head_prob=prob,
                               head_partial=partial)
        ops.mlp_forward(x, mls, ep)
        del packed
        return hs
    h = x
    for i, lin in enumerate(linears):
        last = i == len(linears) - 1
        y = hs[i + 1]
        if last and lin.out_features <= 256:
            ep = ops.make_epilogue(bias=lin.bias, act="relu", head_w=head_w, head_b=head_b, head_logit=logit,
                                   head_prob=prob, head_partial=partial)
        else:
            ep = ops.make_epilogue(bias=lin.bias, act="relu")
        ops.linear(h, lin.weight, y, epilogue=ep)
        h = y
    if linears[-1].out_features > 256:  # head as its own N = 1 GEMM
        ep = ops.make_epilogue(bias=head_b, head_w=const(dev, 1.0), head_b=const(dev, 0.0), head_logit=logit,
                               head_prob=prob, head_partial=partial)
        ops.linear(h, head_w, None, epilogue=ep)
    return hs


def mlp_relu_backward(dh, hs, linears):
    """Backward of mlp_relu_forward's hidden stack from dL/d(last activation); returns
    (dL/dx, [(dW, db) per layer])."""
    grads = [None] * len(linears)
    for i in range(len(linears) - 1, -1, -1):
        dx, dW, db = ops.linear_backward(dh, hs[i], linears[i].weight, relu_out=hs[i + 1])
        grads[i] = (dW, db)
        dh = dx
    return dh, grads


def zero_grads(weights, device):
    """Zero-filled gradient tensors shaped like `weights`, carved from one flat buffer (one fill) at
    256-B aligned offsets, so the row-vector (float4) scatter kernels apply to every table."""
    offs, total = [], 0
    for w in weights:
        offs.append(total)
        total += (w.numel() + 63) // 64 * 64
    flat = torch.zeros(max(total, 1), device=device, dtype=torch.float32)
    return [flat[o:o + w.numel()].view(w.shape) for o, w in zip(offs, weights)]


def sparse_embedding_grads(weights, sources):
    """nn.Embedding(sparse=True) gradients (model(..., sparse_grad=True)): per table one
    torch.sparse_coo_tensor [V, D] whose indices are the looked-up ids as given (unsorted, with
    duplicates, padded positions included) and whose values are the matching rows of the backward's
    dx, nnz = the number of lookups (static for a fixed batch shape, so the step stays capturable).
    sources[k] lists the (ids, matrix, first column[, second matrix]) lookups that feed table k (the
    value rows are the matrix's, plus the second matrix's where a gradient is kept as two summands); a table fed from
    several places gets their entries concatenated (its id lists by one torch.cat; a table with a
    single lookup keeps the caller's id tensor).  The value rows of all tables are packed into
    one flat buffer by one rk_pack_blocks launch; nothing of a table's size is allocated."""
    dev = weights[0].device
    counts = [sum(look[0].numel() for look in src) for src in sources]
    flat = torch.empty(max(1, sum(n * w.shape[1] for n, w in zip(counts, weights))), device=dev, dtype=torch.float32)
    blocks, grads, o = [], [], 0
    for w, src, n in zip(weights, sources, counts):
        D = w.shape[1]
        vals = flat[o:o + n * D].view(n, D)
        o += n * D
        r = 0
        for ids, mat, col, *add in src:
            blocks.append((mat, col, vals[r:r + ids.numel()], *add))
            r += ids.numel()
        ids = src[0][0].reshape(-1) if len(src) == 1 else torch.cat([look[0].reshape(-1) for look in src])
        grads.append(torch.sparse_coo_tensor(ids.unsqueeze(0), vals, w.shape, check_invariants=False))
    ops.pack_blocks(blocks, ops._lib.raw_stream(dev))
    return grads


def embedding_grads(weights, idx, col0, dx, cols=None, sparse=False):
    """Dense nn.Embedding gradients of the tables whose rows sit side by side in dx from column
    col0 on (or at the given `cols`): one zero-filled flat buffer for all tables (one fill),
    then rk_embedding_backward.  sparse: sparse_embedding_grads of the same lookups instead."""
    if cols is None:
        cols, col = [], col0
        for w in weights:
            cols.append(col)
            col += w.shape[1]
    if sparse:
        return sparse_embedding_grads(weights, [[(i, dx, c)] for i, c in zip(idx, cols)])
    grads = zero_grads(weights, dx.device)
    ops.embedding_backward(ops.table_seg_array(grads, idx, cols), dx.shape[0], dx)
    return grads


def _grad_out(g, like):
    if g is None:
        return None
    return g.to(torch.float32).reshape(like.shape).contiguous()


# ---------------------------------------------------------------- DCN

class _DCNTrain(torch.autograd.Function):
    """DCNModel forward + backward; inputs after the fixed arguments are the module parameters in
    `_dcn_params` order."""

    @staticmethod
    def forward(ctx, model, dense, idx, cw, cb, *params):
        B, dev = dense.shape[0], dense.device
        d = model.input_dim
        segs = ops.dense_table_seg_array(dense, model.num_dense_features, [e.weight for e in model.embeddings.values()],
                                         idx)
        x0 = torch.empty(B, d, device=dev, dtype=torch.float32)
        xl = torch.empty(B, d, device=dev, dtype=torch.float32)
        partial = torch.empty(B, device=dev, dtype=torch.float32)
        w_out = model.output_layer.weight
        ops.dcn_cross(segs, B, d, cw, cb, model.num_cross_layer, w_out.data_ptr(), x0, partial, dev, xl_out=xl)
        logit = torch.empty(B, 1, device=dev, dtype=torch.float32)
        prob = torch.empty(B, 1, device=dev, dtype=torch.float32)
        linears = [m for m in model.dnn if isinstance(m, torch.nn.Linear)]
        hs = mlp_relu_forward(x0, linears, w_out[:, d:], model.output_layer.bias, partial, logit, prob)
        ctx.model = model
        ctx.idx = idx
        ctx.save_for_backward(x0, xl, prob, cw, cb, *hs[1:])
        return prob, logit

    @staticmethod
    def backward(ctx, dprob, dlogit):
        model = ctx.model
        x0, xl, prob, cw, cb, *hidden = ctx.saved_tensors
        hs = [x0] + hidden
        B, d = x0.shape
        dev = x0.device
        w_out = model.output_layer.weight
        dprob, dlogit = _grad_out(dprob, prob), _grad_out(dlogit, prob)
        dxl = torch.empty(B, d, device=dev, dtype=torch.float32)
        dh = torch.empty_like(hs[-1])
        dw_out = torch.empty_like(w_out)
        db_out = torch.empty(1, device=dev, dtype=torch.float32)
        ops.logit_head_backward(dlogit, dprob, prob, xl, hs[-1], w_out, dxl, dh, dw_out, db_out)
        linears = [m for m in model.dnn if isinstance(m, torch.nn.Linear)]
        dx0, lin_grads = mlp_relu_backward(dh, hs, linears)
        ops.dcn_cross_backward(x0, cw, cb, model.num_cross_layer, dxl, dx0, accumulate=True)
        emb_grads = embedding_grads([e.weight for e in model.embeddings.values()], ctx.idx,
                                    model.num_dense_features, dx0, sparse=model.sparse_grad)
        flat = [t for pair in lin_grads for t in pair]
        return (None, None, None, None, None, *emb_grads, *flat, dw_out, db_out)


def _dcn_params(model):
    linears = [m for m in model.dnn if isinstance(m, torch.nn.Linear)]
    return ([e.weight for e in model.embeddings.values()] + [t for l in linears for t in (l.weight, l.bias)]
            + [model.output_layer.weight, model.output_layer.bias])


def dcn_train_forward(model, dense, idx, cw, cb):
    if model.output_layer.bias is None or any(m.bias is None for m in model.dnn if isinstance(m, torch.nn.Linear)):
        raise NotImplementedError("rankops DCN training expects the reference's biased Linear layers")
    return _DCNTrain.apply(model, dense, idx, cw, cb, *_dcn_params(model))


# ---------------------------------------------------------------- DeepCrossing

class _DeepCrossingTrain(torch.autograd.Function):
    """DeepCrossingModel forward + backward (deepcrossing.py:146-163): gather, residual units
    (per-call Linear(d, I) / Linear(I, d) drawn like the reference — not module parameters, so
    only the gradient w.r.t. their input is propagated), output_layer + sigmoid."""

    @staticmethod
    def forward(ctx, model, dense, idx, units, *params):
        B, dev = dense.shape[0], dense.device
        d, I = model.input_dim, model.residual_internal_dim
        segs = [ops.dense_segment(dense, model.num_dense_features, 0)]
        col = model.num_dense_features
        for emb, i in zip(model.embeddings.values(), idx):
            segs.append(ops.table_segment(emb.weight, i, col))
            col += emb.embedding_dim
        x0 = torch.empty(B, d, device=dev, dtype=torch.float32)
        ops.concat_gather(segs, B, x0)
        logit = torch.empty(B, 1, device=dev, dtype=torch.float32)
        prob = torch.empty(B, 1, device=dev, dtype=torch.float32)
        head = dict(head_w=model.output_layer.weight, head_b=model.output_layer.bias, head_logit=logit,
                    head_prob=prob)
        acts = []  # h_1, y_1, h_2, y_2, ...
        for _ in units:
            acts += [torch.empty(B, I, device=dev, dtype=torch.float32),
                     torch.empty(B, d, device=dev, dtype=torch.float32)]
        widths = [w for _ in units for w in (I, d)]
        if units and common.FUSED_MLP and fused_mlp_fits(d, widths):
            pack = ops.pack_mlp_weight if torch.cuda.is_current_stream_capturing() else PACKED
            packed = [(pack(w1), pack(w2)) for w1, b1, w2, b2 in units]
            layers = []
            for (w1, b1, w2, b2), (p1, p2), j in zip(units, packed, range(0, len(acts), 2)):
                layers.append(ops.make_mlp_layer(w1, p1, bias=b1, act="relu", store=acts[j], ld_store=I))
                layers.append(ops.make_mlp_layer(w2, p2, bias=b2, act="relu", residual=1, store=acts[j + 1],
                                                 ld_store=d))
            ops.mlp_forward(x0, layers, ops.make_epilogue(**head))
            del packed
        else:
            x = x0
            for (w1, b1, w2, b2), j in zip(units, range(0, len(acts), 2)):
                ops.linear(x, w1, acts[j], epilogue=ops.make_epilogue(bias=b1, act="relu"))
                ops.linear(acts[j], w2, acts[j + 1], epilogue=ops.make_epilogue(
                    bias=b2, residual=x, ld_residual=x.stride(0), act="relu"))
                x = acts[j + 1]
            ep = ops.make_epilogue(bias=model.output_layer.bias, head_w=const(dev, 1.0), head_b=const(dev, 0.0),
                                   head_logit=logit, head_prob=prob)
            ops.linear(x, model.output_layer.weight, None, epilogue=ep)
        ctx.model, ctx.idx = model, idx
        ctx.save_for_backward(x0, prob, *[t for u in units for t in (u[0], u[2])], *acts)
        return prob, logit

    @staticmethod
    def backward(ctx, dprob, dlogit):
        model = ctx.model
        x0, prob, *rest = ctx.saved_tensors
        n = (len(rest)) // 4
        ws, acts = rest[:2 * n], rest[2 * n:]
        B, d = x0.shape
        dev = x0.device
        last = acts[-1] if n else x0
        dy = torch.empty(B, d, device=dev, dtype=torch.float32)
        dw_out = torch.empty_like(model.output_layer.weight)
        db_out = torch.empty(1, device=dev, dtype=torch.float32)
        ops.logit_head_backward(_grad_out(dlogit, prob), _grad_out(dprob, prob), prob, last, None,
                                model.output_layer.weight, dy, None, dw_out, db_out)
        for u in range(n - 1, -1, -1):
            w1, w2 = ws[2 * u], ws[2 * u + 1]
            h, y = acts[2 * u], acts[2 * u + 1]
            I = h.shape[1]
            # y = relu(x + h W2^T + b2), h = relu(x W1^T + b1)
            dh = torch.empty(B, I, device=dev, dtype=torch.float32)
            ops.gemm(False, True, B, I, d, dy, d, w2, I, dh, A_mask=y)           # dz2 W2
            dx = torch.empty(B, d, device=dev, dtype=torch.float32)
            ops.relu_backward(dy, y, dx)                                        # residual path
            ops.gemm(False, True, B, d, I, dh, I, w1, d, dx, A_mask=h, accumulate=True)  # + dz1 W1
            dy = dx
        emb_grads = embedding_grads([e.weight for e in model.embeddings.values()], ctx.idx,
                                    model.num_dense_features, dy, sparse=model.sparse_grad)
        return (None, None, None, None, *emb_grads, dw_out, db_out)


def deepcrossing_train_forward(model, dense, idx, units):
    params = [e.weight for e in model.embeddings.values()] + [model.output_layer.weight, model.output_layer.bias]
    return _DeepCrossingTrain.apply(model, dense, idx, units, *params)


# ---------------------------------------------------------------- DeepFM

def deep_units(layers):
    """(Linear, BatchNorm1d or None, ReLU?, dropout p) per unit of a Linear/[BN]/ReLU/[Dropout]
    sequence (deepfm.py:100-109)."""
    units = []
    for m in layers:
        if isinstance(m, torch.nn.Linear):
            units.append([m, None, False, 0.0])
        elif isinstance(m, torch.nn.BatchNorm1d):
            units[-1][1] = m
        elif isinstance(m, torch.nn.ReLU):
            units[-1][2] = True
        elif isinstance(m, torch.nn.Dropout):
            units[-1][3] = float(m.p) if m.training else 0.0
        else:
            raise NotImplementedError(f"rankops training: unsupported layer {type(m).__name__}")
    for lin, bn, relu, _ in units:
        if bn is not None and (bn.momentum is None or not bn.training):
            raise NotImplementedError("rankops training: BatchNorm1d needs a numeric momentum and train mode")
    return units


class DropoutStreams:
    """Per-model dropout stream counter on the device (advanced by rk_rng_next once per train
    forward, so hipGraph replays draw fresh masks) and the seed (torch.initial_seed() when first
    used: seeded runs repeat their masks)."""

    def __init__(self):
        self.counter = None
        self.seed = None

    def next(self, device):
        if self.counter is None or self.counter.device != device:
            self.counter = torch.zeros(1, dtype=torch.int64, device=device)
            self.seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        slot = torch.empty(1, dtype=torch.int64, device=device)
        ops.rng_next(self.counter, slot)
        return self.seed, slot


def deep_stack_forward(x, units, seed, slot):
    """Train-mode Linear -> [BN] -> ReLU -> [Dropout] stack; returns per-unit saved tensors."""
    B, dev = x.shape[0], x.device
    saved = []
    h = x
    for u, unit in enumerate(units):
        lin, bn, act, p = unit[:4]
        slope = unit[4] if len(unit) > 4 else 0.0
        n = lin.out_features
        z = torch.empty(B, n, device=dev, dtype=torch.float32)
        ops.gemm(False, False, B, n, lin.in_features, h, h.stride(0), lin.weight, lin.weight.stride(0), z)
        y = torch.empty(B, n, device=dev, dtype=torch.float32)
        mean = torch.empty(n, device=dev, dtype=torch.float32)
        invstd = torch.empty(n, device=dev, dtype=torch.float32)
        ws = torch.empty(2 * n, device=dev, dtype=torch.float64)
        ops.bn_act_train_forward(z, lin.bias, bn, act, p, seed + u, slot, y, mean, invstd, ws, slope=slope)
        saved.append((z, y, mean, invstd))
        h = y
    return saved


def deep_stack_backward(dy, x, units, saved, seed, slot):
    """Backward of deep_stack_forward from dL/d(last output); returns (dL/dx, per-unit grads
    [dW, db, (dgamma, dbeta)])."""
    B, dev = x.shape[0], x.device
    grads = [None] * len(units)
    for u in range(len(units) - 1, -1, -1):
        lin, bn, act, p = units[u][:4]
        slope = units[u][4] if len(units[u]) > 4 else 0.0
        z, y, mean, invstd = saved[u]
        n, K = lin.out_features, lin.in_features
        h_in = saved[u - 1][1] if u > 0 else x
        dz = torch.empty(B, n, device=dev, dtype=torch.float32)
        ws = torch.empty(2 * n, device=dev, dtype=torch.float64)
        dg = torch.empty(n, device=dev, dtype=torch.float32) if bn is not None and bn.weight is not None else None
        dbt = torch.empty(n, device=dev, dtype=torch.float32) if bn is not None and bn.bias is not None else None
        ops.bn_act_backward(dy, z, lin.bias, bn, act, p, seed + u, slot, mean, invstd, ws, dz, dg, dbt, slope=slope)
        dW = torch.empty(n, K, device=dev, dtype=torch.float32)
        db = torch.empty(n, device=dev, dtype=torch.float32)
        ops.gemm(True, True, n, K, B, dz, dz.stride(0), h_in, h_in.stride(0), dW, row_sums=db)
        dx = torch.empty(B, K, device=dev, dtype=torch.float32)
        ops.gemm(False, True, B, K, n, dz, dz.stride(0), lin.weight, lin.weight.stride(0), dx)
        g = [dW, db if lin.bias is not None else None]
        if bn is not None:
            g += [t for t in (dg, dbt) if t is not None]
        grads[u] = g
        dy = dx
    return dy, grads


def _unit_params(units):
    out = []
    for unit in units:
        lin, bn = unit[0], unit[1]
        out += [lin.weight] + ([lin.bias] if lin.bias is not None else [])
        if bn is not None:
            out += [t for t in (bn.weight, bn.bias) if t is not None]
    return out


def deepfm_tail_forward(ctx, model, deep_in, fm1, fm2):
    """The train forward after the FM front end, shared by DeepFM and ShardedDeepFM (deepfm.py:142-151):
    the Linear -> BN -> ReLU -> Dropout units, deep_output_layer, final_layer + sigmoid.  Saves on ctx
    what deepfm_tail_backward reads; returns (prob, total, deep)."""
    B, dev = deep_in.shape[0], deep_in.device
    units = deep_units(model.deep_layers)
    seed, slot = model._dropout.next(dev)
    saved = deep_stack_forward(deep_in, units, seed, slot)
    last = saved[-1][1] if saved else deep_in
    deep = torch.empty(B, 1, device=dev, dtype=torch.float32)
    total = torch.empty(B, 1, device=dev, dtype=torch.float32)
    prob = torch.empty(B, 1, device=dev, dtype=torch.float32)
    ep = ops.make_epilogue(head_w=model.deep_output_layer.weight, head_b=model.deep_output_layer.bias, fm1=fm1,
                           fm2=fm2, final_w=model.final_layer.weight, final_b=model.final_layer.bias,
                           head_aux=deep, head_logit=total, head_prob=prob)
    ops.mlp_forward(last, [], ep)
    ctx.model, ctx.units, ctx.seed = model, units, seed
    ctx.save_for_backward(deep_in, fm1, fm2, deep, prob, slot, *[t for s in saved for t in s])
    return prob, total, deep


def deepfm_tail_backward(ctx, dprob, dtotal, dfm1_o, dfm2_o, ddeep_o):
    """Backward of deepfm_tail_forward: (deep_in, dfm1, dfm2, dL/d deep_in, the dense parameters'
    gradients in deepfm_dense_params order)."""
    model, units = ctx.model, ctx.units
    deep_in, fm1, fm2, deep, prob, slot, *flat = ctx.saved_tensors
    saved = [tuple(flat[4 * u:4 * u + 4]) for u in range(len(units))]
    B, dev = deep_in.shape[0], deep_in.device
    go = [_grad_out(g, prob) for g in (dprob, dtotal, dfm1_o, dfm2_o, ddeep_o)]
    dfm1 = torch.empty(B, 1, device=dev, dtype=torch.float32)
    dfm2 = torch.empty(B, 1, device=dev, dtype=torch.float32)
    ddeep = torch.empty(B, 1, device=dev, dtype=torch.float32)
    dfinal_w = torch.empty_like(model.final_layer.weight)
    dfinal_b = torch.empty(1, device=dev, dtype=torch.float32)
    ops.fm_combine_backward(*go, prob, fm1, fm2, deep, model.final_layer.weight, dfm1, dfm2, ddeep, dfinal_w,
                            dfinal_b)
    last = saved[-1][1] if saved else deep_in
    dy = torch.empty_like(last)
    dw_do = torch.empty_like(model.deep_output_layer.weight)
    db_do = torch.empty(1, device=dev, dtype=torch.float32)
    ops.logit_head_backward(ddeep, None, None, last, None, model.deep_output_layer.weight, dy, None, dw_do, db_do)
    d_deep_in, unit_grads = deep_stack_backward(dy, deep_in, units, saved, ctx.seed, slot)
    flat_g = [t for g in unit_grads for t in g if t is not None]
    return deep_in, dfm1, dfm2, d_deep_in, (*flat_g, dw_do, db_do, dfinal_w, dfinal_b)


def deepfm_dense_params(model, units):
    """The replicated (non-table) parameters of a DeepFM, in the order of deepfm_tail_backward's gradients."""
    if model.deep_output_layer.bias is None or model.final_layer.bias is None:
        raise NotImplementedError("rankops DeepFM training expects the reference's biased output layers")
    return _unit_params(units) + [model.deep_output_layer.weight, model.deep_output_layer.bias,
                                  model.final_layer.weight, model.final_layer.bias]


class _DeepFMTrain(torch.autograd.Function):
    """DeepFM forward + backward in train mode (deepfm.py:121-151): FM gather, Linear -> BN(batch
    statistics) -> ReLU -> Dropout units, deep_output_layer, final_layer + sigmoid."""

    @staticmethod
    def forward(ctx, model, names, idx, *params):
        D = model.embedding_dim
        F = len(names)
        B, dev = idx[0].shape[0], idx[0].device
        second = ops.table_seg_array([model.second_order_embeddings[n].weight for n in names], idx,
                                     [f * D for f in range(F)])
        first = ops.table_seg_array([model.first_order_embeddings[n].weight for n in names], idx, list(range(F)))
        deep_in = torch.empty(B, F * D, device=dev, dtype=torch.float32)
        fm1 = torch.empty(B, 1, device=dev, dtype=torch.float32)
        fm2 = torch.empty(B, 1, device=dev, dtype=torch.float32)
        ops.fm_gather(second, first, D, B, deep_in, fm1, fm2)
        prob, total, deep = deepfm_tail_forward(ctx, model, deep_in, fm1, fm2)
        ctx.names, ctx.idx = names, idx
        return prob, total, fm1, fm2, deep

    @staticmethod
    def backward(ctx, dprob, dtotal, dfm1_o, dfm2_o, ddeep_o):
        model = ctx.model
        deep_in, dfm1, dfm2, d_deep_in, dense_grads = deepfm_tail_backward(ctx, dprob, dtotal, dfm1_o, dfm2_o, ddeep_o)
        B, dev = deep_in.shape[0], deep_in.device
        D, F = model.embedding_dim, len(ctx.names)
        d_second = torch.empty(B, F * D, device=dev, dtype=torch.float32)
        ops.fm_backward(deep_in, d_deep_in, dfm2, F, D, d_second)
        w2 = [model.second_order_embeddings[n].weight for n in ctx.names]
        w1 = [model.first_order_embeddings[n].weight for n in ctx.names]
        if model.sparse_grad:  # both table sets in one packing launch
            g = sparse_embedding_grads(w1 + w2, [[(i, dfm1, 0)] for i in ctx.idx]
                                       + [[(i, d_second, f * D)] for f, i in enumerate(ctx.idx)])
            g1, g2 = g[:F], g[F:]
        else:
            g2 = embedding_grads(w2, ctx.idx, 0, d_second)
            g1 = embedding_grads(w1, ctx.idx, 0, dfm1, cols=[0] * F)
        return (None, None, None, *g1, *g2, *dense_grads)


def deepfm_train_forward(model, names, idx):
    units = deep_units(model.deep_layers)
    dense = deepfm_dense_params(model, units)
    params = ([model.first_order_embeddings[n].weight for n in names]
              + [model.second_order_embeddings[n].weight for n in names] + dense)
    return _DeepFMTrain.apply(model, names, idx, *params)


class _ShardedDeepFMTrain(torch.autograd.Function):
    """ShardedDeepFM's train forward + the local half of its backward (rankops/sharded.py): the
    received row blocks are assembled (rk_shard_fm_assemble) and run through DeepFM's tail; the
    backward hands autograd the local gradients of the replicated dense parameters and leaves the
    table gradients, packed for the gradient all-to-all by rk_shard_fm_backward_pack and already
    scaled by 1 / world, on the module for sync_gradients().  No collective runs in here: autograd
    calls backward from its own thread, where neither a barrier nor the caller's stream is safe."""

    @staticmethod
    def forward(ctx, model, recv_rows, recv_idx, B, *params):
        D, F, dev = model.embedding_dim, len(model.fields), recv_rows.device
        deep_in = torch.empty(B, F * D, device=dev, dtype=torch.float32)
        fm1 = torch.empty(B, 1, device=dev, dtype=torch.float32)
        fm2 = torch.empty(B, 1, device=dev, dtype=torch.float32)
        if B:
            ops.shard_fm_assemble(recv_rows, F, model.world, D, deep_in, fm1, fm2)
        prob, total, deep = deepfm_tail_forward(ctx, model, deep_in, fm1, fm2)
        ctx.recv_idx = recv_idx
        return prob, total, fm1, fm2, deep

    @staticmethod
    def backward(ctx, dprob, dtotal, dfm1_o, dfm2_o, ddeep_o):
        model = ctx.model
        if model._pending is not None:
            raise RuntimeError("ShardedDeepFM: a train backward is already outstanding; call sync_gradients() "
                               "before the next backward (one step at a time)")
        deep_in, dfm1, dfm2, d_deep_in, dense_grads = deepfm_tail_backward(ctx, dprob, dtotal, dfm1_o, dfm2_o, ddeep_o)
        B = deep_in.shape[0]
        send = torch.empty(sum(model.train_row_splits(B)[0]), device=deep_in.device, dtype=torch.float32)
        if B:
            ops.shard_fm_backward_pack(deep_in, d_deep_in, dfm2, dfm1, 1.0 / model.world, len(model.fields),
                                       model.world, model.embedding_dim, send)
        model._pending = (send, ctx.recv_idx, B)
        return (None, None, None, None, *dense_grads)


def sharded_deepfm_train_forward(model, recv_rows, recv_idx, B):
    units = deep_units(model.deep_layers)
    return _ShardedDeepFMTrain.apply(model, recv_rows, recv_idx, B, *deepfm_dense_params(model, units))


# ---------------------------------------------------------------- xDeepFM

class _NoSave:
    """Stands in for an autograd context where a train-mode forward keeps nothing (no_grad)."""

    def save_for_backward(self, *tensors):
        pass


def _xdeepfm_front(model, names, idx, maps: bool):
    """The train forward's first launches: both CIN weight images packed on the stream into the
    model's own buffers (a hipGraph replay repacks the weights Adam just stepped; common.CIN_PACKED
    decides on the host and would freeze an image into the graph), then rk_cin_forward_train (or
    rk_cin_forward when no maps are kept).  Returns (deep_in, fm1, cin_logit, pooled, maps, images_t)."""
    D, F = model.embedding_dim, len(names)
    B, dev = idx[0].shape[0], idx[0].device
    second = ops.table_seg_array([model.second_order_embeddings[n].weight for n in names], idx,
                                 [f * D for f in range(F)])
    first = ops.table_seg_array([model.first_order_embeddings[n].weight for n in names], idx, list(range(F)))
    own = model.__dict__.setdefault("_cin_train_images", {})
    images, images_t = [], []
    for k, c in enumerate(model.cin_layers):
        own[k, 0] = ops.pack_cin_weight(c.weight, out=own.get((k, 0)))
        images.append(own[k, 0])
        if maps:
            own[k, 1] = ops.pack_cin_weight_t(c.weight, F, out=own.get((k, 1)))
            images_t.append(own[k, 1])
    biases = [c.bias for c in model.cin_layers]
    f32 = dict(device=dev, dtype=torch.float32)
    deep_in = torch.empty(B, F * D, **f32)
    fm1, cin_logit = torch.empty(B, 1, **f32), torch.empty(B, 1, **f32)
    sizes = model.cin_layer_sizes
    out = dict(out_w=model.cin_output_layer.weight, out_b=model.cin_output_layer.bias, deep_in=deep_in, fm1=fm1,
               cin_logit=cin_logit)
    if not maps:
        ops.cin_forward(second, first, D, B, images, biases, sizes, model.cin_activation, dev, **out)
        return deep_in, fm1, cin_logit, None, None, None
    pooled = torch.empty(B, sum(sizes), **f32)
    saved = torch.empty(B, sum(sizes), D, **f32)
    ops.cin_forward_train(second, first, D, B, images, biases, sizes, model.cin_activation, dev, saved, pooled=pooled,
                          **out)
    return deep_in, fm1, cin_logit, pooled, saved, images_t


class _XDeepFMTrain(torch.autograd.Function):
    """XDeepFM forward + backward in train mode: rk_cin_forward_train (gather, first-order sum, the
    CIN with its maps kept, pooling, cin_output_layer), DeepFM's train tail with fm2 = cin_logit;
    backward: the tail, cin_output_layer (rk_logit_head_backward on the kept pooled), rk_cin_backward
    (dx0 + the deep stack's input gradient in its epilogue), rk_cin_wgrad, the embedding gradients.
    Inputs after the fixed arguments: first-order tables, second-order tables, deepfm_dense_params,
    the CIN weights, the CIN biases, cin_output_layer's weight and bias."""

    @staticmethod
    def forward(ctx, model, names, idx, *params):
        deep_in, fm1, cin_logit, pooled, maps, images_t = _xdeepfm_front(model, names, idx, True)
        prob, total, deep = deepfm_tail_forward(ctx, model, deep_in, fm1, cin_logit)
        ctx.names, ctx.idx = names, idx
        ctx.cin = (pooled, maps, images_t)
        return prob, total, fm1, cin_logit, deep

    @staticmethod
    def backward(ctx, dprob, dtotal, dfm1_o, dcin_o, ddeep_o):
        model = ctx.model
        deep_in, dfm1, dcin, d_deep_in, dense_grads = deepfm_tail_backward(ctx, dprob, dtotal, dfm1_o, dcin_o, ddeep_o)
        pooled, maps, images_t = ctx.cin
        B, dev = deep_in.shape[0], deep_in.device
        D, F = model.embedding_dim, len(ctx.names)
        out_w = model.cin_output_layer.weight
        d_out_w = torch.empty_like(out_w)
        d_out_b = torch.empty(1, device=dev, dtype=torch.float32)
        ops.logit_head_backward(dcin, None, None, pooled, None, out_w, None, None, d_out_w, d_out_b)
        sizes = model.cin_layer_sizes
        d_second, dy = ops.cin_backward(deep_in, F, D, images_t, sizes, model.cin_activation, maps, dlogit=dcin,
                                        out_w=out_w, dx0_add=d_deep_in)
        ws = model.__dict__.get("_cin_wgrad_ws")
        if ws is None or ws.device != dev:
            ws = model.__dict__["_cin_wgrad_ws"] = ops.cin_wgrad_workspace(F, sizes, dev)
        dws, dbs = ops.cin_wgrad(deep_in, F, D, sizes, maps, dy, workspace=ws)
        dws = [g.view(c.weight.shape) for g, c in zip(dws, model.cin_layers)]
        w2 = [model.second_order_embeddings[n].weight for n in ctx.names]
        w1 = [model.first_order_embeddings[n].weight for n in ctx.names]
        if model.sparse_grad:  # both table sets in one packing launch
            g = sparse_embedding_grads(w1 + w2, [[(i, dfm1, 0)] for i in ctx.idx]
                                       + [[(i, d_second, f * D)] for f, i in enumerate(ctx.idx)])
            g1, g2 = g[:F], g[F:]
        else:
            g2 = embedding_grads(w2, ctx.idx, 0, d_second)
            g1 = embedding_grads(w1, ctx.idx, 0, dfm1, cols=[0] * F)
        return (None, None, None, *g1, *g2, *dense_grads, *dws, *dbs, d_out_w, d_out_b)


def xdeepfm_train_forward(model, names, idx, grad: bool = True):
    """XDeepFM train-mode forward: (probability, total_logit, linear_logit, cin_logit, deep_logit)
    attached to _XDeepFMTrain when `grad`; otherwise the same launches with nothing kept."""
    if not grad:
        deep_in, fm1, cin_logit, *_ = _xdeepfm_front(model, names, idx, False)
        prob, total, deep = deepfm_tail_forward(_NoSave(), model, deep_in, fm1, cin_logit)
        return prob, total, fm1, cin_logit, deep
    units = deep_units(model.deep_layers)
    dense = deepfm_dense_params(model, units)
    if any(c.bias is None for c in model.cin_layers) or model.cin_output_layer.bias is None:
        raise NotImplementedError("rankops XDeepFM training expects biased CIN and output layers")
    params = ([model.first_order_embeddings[n].weight for n in names]
              + [model.second_order_embeddings[n].weight for n in names] + dense
              + [c.weight for c in model.cin_layers] + [c.bias for c in model.cin_layers]
              + [model.cin_output_layer.weight, model.cin_output_layer.bias])
    return _XDeepFMTrain.apply(model, names, idx, *params)


# ---------------------------------------------------------------- MMoE

def _mmoe_lists(model):
    """(experts, gates, towers) of a rankops.MMoE in ops.mmoe_backward's form, detached."""
    lin = model._linears
    experts = [[(l.weight.detach(), l.bias) for l in lin(seq)] for seq in model.experts]
    gates = [(g.weight.detach(), g.bias) for g in model.gates]
    towers = [([(l.weight.detach(), l.bias) for l in lin(seq)], (o.weight.detach().reshape(-1), o.bias))
              for seq, o in zip(model.towers, model.tower_outputs)]
    return experts, gates, towers


def _mmoe_front(model, dense, names, idx):
    """The train forward: every image the kernel reads repacked on the stream into the model's own buffers
    (one torch.cat for the stacked layer-0 / gate weight, one for the gate biases, one
    rk_mlp_pack_weights for all images; a hipGraph replay follows the optimizer), the dropout stream
    advanced (rk_rng_next), then rk_mmoe_forward_train.  Returns (shape, saved buffers)."""
    B, dev = dense.shape[0], dense.device
    E, K = model.num_experts, len(model.task_names)
    sh = ops.MmoeShape(model.input_dim, E, K, model.expert_hidden_units, model.tower_hidden_units, True)
    experts, gates, towers = _mmoe_lists(model)
    wst = ops.mmoe_stacked_weight(sh, experts, gates)
    gate_b = torch.cat([g.bias.detach() for g in model.gates], 0)
    own = model.__dict__.setdefault("_train_images", {})
    if own.get("device") != dev:
        own.clear()
        own["device"] = dev
    pairs, stacks, tstacks = [], [], []

    def image(key, w):
        img = own.get(key)
        if img is None:
            img = own[key] = ops.mlp_image(w.shape[0], w.shape[1], dev)
        pairs.append((w, img))
        return img
    for e, layers in enumerate(experts):
        stacks.append([(image(("e", e, l), w), b, w.shape[0], "relu") for l, (w, b) in enumerate(layers)])
    for k, (hidden, _) in enumerate(towers):
        tstacks.append([(image(("t", k, l), w), b, w.shape[0], "relu") for l, (w, b) in enumerate(hidden)])
    gate_rows = wst[E * ops.p4(sh.eu[0]):E * ops.p4(sh.eu[0]) + K * E, :sh.width]  # the stacked gates: wst's tail
    gate_image = image("g", gate_rows)
    stream = ops._lib.raw_stream(dev)
    ops.pack_mlp_weights(pairs, stream)
    p = float(model.dropout_rate)
    seed, slot = 0, None
    if p > 0:
        seed, slot = model.__dict__.setdefault("_dropout", DropoutStreams()).next(dev)
    heads = [(w, b) for _, (w, b) in towers]
    s = ops.mmoe_forward_train(model._segments(dense, names, idx), sh, B, stacks, gate_image, gate_b, tstacks, heads,
                               dev, p, seed, slot)
    s["weights"] = (experts, gates, towers, wst)
    s["dropout"] = (seed, slot)
    return sh, s


class _MMoETrain(torch.autograd.Function):
    """MMoE forward + backward in train mode: rk_mmoe_forward_train (one launch: gather, gates, experts with
    dropout, mix, towers, heads, every activation kept), then ops.mmoe_backward (heads, towers, mix and
    gates, experts, the stacked layer 0, each a fixed number of launches whatever E and K) and the
    embedding gradients.  Inputs after the fixed arguments: the tables, then every expert Linear's
    (weight, bias) expert-major, the gates', every tower Linear's, the output layers'."""

    @staticmethod
    def forward(ctx, model, dense, names, idx, *params):
        sh, s = _mmoe_front(model, dense, names, idx)
        ctx.model, ctx.sh, ctx.s, ctx.names, ctx.idx, ctx.B = model, sh, s, names, idx, dense.shape[0]
        ctx.set_materialize_grads(False)
        return s["probs"], s["logits"]

    @staticmethod
    def backward(ctx, dprob, dlogit):
        model, sh, s, B = ctx.model, ctx.sh, ctx.s, ctx.B
        dev = s["x"].device
        experts, gates, towers, wst = s["weights"]
        if dprob is None and dlogit is None:
            dlogit = torch.zeros(B, sh.K, device=dev, dtype=torch.float32)
        dx, eg, gg, tg = ops.mmoe_backward(sh, B, s, wst, experts, gates, towers, float(model.dropout_rate), None,
                                           _grad_out(dlogit, s["logits"]), _grad_out(dprob, s["probs"]), True, dev)
        tables = [model.embeddings[n].weight for n in ctx.names]
        g_tab = embedding_grads(tables, ctx.idx, model.num_dense_features, dx, sparse=model.sparse_grad)
        out = list(g_tab)
        for e in range(sh.E):
            for l in range(len(sh.eu)):
                out += list(eg[e][l])
        for k in range(sh.K):
            out += list(gg[k])
        for k in range(sh.K):
            for l in range(len(sh.tu)):
                out += list(tg[k][0][l])
        for k in range(sh.K):
            out += [tg[k][1][0], tg[k][1][1]]
        return (None, None, None, None, *out)


class _MultiTaskEmpty(torch.autograd.Function):
    """A multi-task model's (MMoE, PLE, ESMM) train forward over an empty batch: empty outputs attached to the parameters, whose
    gradients are zeros (what the reference's loop gets from autograd); no kernel of the engine runs."""

    @staticmethod
    def forward(ctx, K, device, *params):
        ctx.params = params
        return (torch.empty(0, K, device=device, dtype=torch.float32),
                torch.empty(0, K, device=device, dtype=torch.float32))

    @staticmethod
    def backward(ctx, dprob, dlogit):
        return (None, None, *[torch.zeros_like(p) for p in ctx.params])


def _mmoe_params(model, names):
    lin = model._linears
    params = [model.embeddings[n].weight for n in names]
    for seq in model.experts:
        for l in lin(seq):
            params += [l.weight, l.bias]
    for g in model.gates:
        params += [g.weight, g.bias]
    for seq in model.towers:
        for l in lin(seq):
            params += [l.weight, l.bias]
    for o in model.tower_outputs:
        params += [o.weight, o.bias]
    return params


def multitask_train_forward(model, dense, names, idx, grad: bool = True):
    """Train-mode forward of a multi-task model (MMoE, PLE, ESMM): (probabilities [B, K], logits [B, K]) attached
    to the model's autograd function when `grad`; otherwise the same launches with nothing kept.  An empty
    batch returns empty outputs (attached, with zero gradients, when `grad`) without running the engine."""
    front, fn, params = {"MMoE": (_mmoe_front, _MMoETrain, _mmoe_params),
                         "PLE": (_ple_front, _PLETrain, _ple_params),
                         "ESMM": (_esmm_front, _ESMMTrain, _esmm_params)}[model.NAME]
    if dense.shape[0] == 0:
        if not grad:
            return common.empty_rows(dense.device, 2, (0, len(model.task_names)))
        return _MultiTaskEmpty.apply(len(model.task_names), dense.device,
                                     *[p for p in model.parameters() if p.requires_grad])
    if not grad:
        _, s = front(model, dense, names, idx)
        return s["probs"], s["logits"]
    return fn.apply(model, dense, names, idx, *params(model, names))


# ---------------------------------------------------------------- PLE

def _ple_lists(model):
    """(levels, towers) of a rankops.PLE in ops.ple_backward's form, detached."""
    lin = model._linears
    levels = [([[(l.weight.detach(), l.bias) for l in lin(seq)] for seq in level.stacks()],
               [(g.weight.detach(), g.bias) for g in level.all_gates()]) for level in model.levels]
    towers = [([(l.weight.detach(), l.bias) for l in lin(seq)], (o.weight.detach().reshape(-1), o.bias))
              for seq, o in zip(model.towers, model.tower_outputs)]
    return levels, towers


def _ple_front(model, dense, names, idx):
    """The train forward, as _mmoe_front: every image the kernel reads repacked on the stream into the
    model's own buffers (one rk_mlp_pack_weights for all of them, so the addresses and with them the
    device layer table are the same every step and a hipGraph replay follows the optimizer), the
    per-level stacked first-layer / gate weights assembled (ops.ple_stacked_weights), the dropout stream
    advanced (rk_rng_next), then rk_ple_forward_train.  Returns (shape, saved buffers)."""
    B, dev = dense.shape[0], dense.device
    K = len(model.task_names)
    sh = ops.PleShape(model.input_dim, model.num_levels, K, model.num_specific_experts, model.num_shared_experts,
                      model.expert_hidden_units, model.tower_hidden_units, True)
    levels, towers = _ple_lists(model)
    wst = ops.ple_stacked_weights(sh, levels)
    own = model.__dict__.setdefault("_train_images", {})
    if own.get("device") != dev:
        own.clear()
        own["device"] = dev
    pairs = []

    def image(key, w):
        img = own.get(key)
        if img is None:
            img = own[key] = ops.mlp_image(w.shape[0], w.shape[1], dev)
        pairs.append((w, img))
        return img
    experts, gates = [], []
    for j, (stacks, lgates) in enumerate(levels):
        experts += [(image(("e", j, i, l), w), b) for i, layers in enumerate(stacks) for l, (w, b) in enumerate(layers)]
        gates += [(image(("g", j, q), w), b) for q, (w, b) in enumerate(lgates)]
        if len(lgates) == K:  # the last level: the shared gate's slot is never read
            gates.append((gates[-1][0], None))
    tw = [(image(("t", k, l), w), b) for k, (hidden, _) in enumerate(towers) for l, (w, b) in enumerate(hidden)]
    heads = [(o.weight.detach(), o.bias) for o in model.tower_outputs]
    stream = ops._lib.raw_stream(dev)
    ops.pack_mlp_weights(pairs, stream)
    p = float(model.dropout_rate)
    seed, slot = 0, None
    if p > 0:
        seed, slot = model.__dict__.setdefault("_dropout", DropoutStreams()).next(dev)
    s = ops.ple_forward_train(model._segments(dense, names, idx), sh, B, experts + gates + tw + heads, dev, p, seed, slot)
    s["weights"] = (levels, towers, wst)
    s["dropout"] = (seed, slot)
    return sh, s


class _PLETrain(torch.autograd.Function):
    """PLE forward + backward in train mode: rk_ple_forward_train (one launch: gather, every level's gates,
    experts with dropout and mixtures, towers, heads, every activation kept), then ops.ple_backward and the
    embedding gradients.  Inputs after the fixed arguments: the tables, then per level every stack Linear's
    (weight, bias) stack-major and the gates', then per tower its Linears' and its output layer's."""

    @staticmethod
    def forward(ctx, model, dense, names, idx, *params):
        sh, s = _ple_front(model, dense, names, idx)
        ctx.model, ctx.sh, ctx.s, ctx.names, ctx.idx, ctx.B = model, sh, s, names, idx, dense.shape[0]
        ctx.set_materialize_grads(False)
        return s["probs"], s["logits"]

    @staticmethod
    def backward(ctx, dprob, dlogit):
        model, sh, s, B = ctx.model, ctx.sh, ctx.s, ctx.B
        dev = s["x"].device
        levels, towers, wst = s["weights"]
        if dprob is None and dlogit is None:
            dlogit = torch.zeros(B, sh.K, device=dev, dtype=torch.float32)
        dx, lg, tg = ops.ple_backward(sh, B, s, wst, levels, towers, float(model.dropout_rate), None,
                                      _grad_out(dlogit, s["logits"]), _grad_out(dprob, s["probs"]), True, dev)
        tables = [model.embeddings[n].weight for n in ctx.names]
        g_tab = embedding_grads(tables, ctx.idx, model.num_dense_features, dx, sparse=model.sparse_grad)
        return (None, None, None, None, *g_tab, *ops.ple_flat_grads(sh, lg, tg))  # (_ple_params' order)


def _ple_params(model, names):
    lin = model._linears
    params = [model.embeddings[n].weight for n in names]
    for level in model.levels:
        for seq in level.stacks():
            for l in lin(seq):
                params += [l.weight, l.bias]
        for g in level.all_gates():
            params += [g.weight, g.bias]
    for seq, o in zip(model.towers, model.tower_outputs):
        for l in lin(seq):
            params += [l.weight, l.bias]
        params += [o.weight, o.bias]
    return params


# ---------------------------------------------------------------- ESMM

def _esmm_front(model, dense, names, idx):
    """The train forward, as _mmoe_front: every image the kernel reads repacked on the stream into the
    model's own buffers (one rk_mlp_pack_weights for all of them, one torch.cat for the stacked layer-0
    weight; a hipGraph replay follows the optimizer), the dropout stream advanced (rk_rng_next), then
    rk_esmm_forward_train.  Returns (shape, saved buffers)."""
    B, dev = dense.shape[0], dense.device
    lin = model._linears
    sh = ops.EsmmShape(model.input_dim, len(model.task_names), model.tower_hidden_units)
    towers = [([(l.weight.detach(), l.bias) for l in lin(seq)], (o.weight.detach().reshape(-1), o.bias))
              for seq, o in zip(model.towers, model.tower_outputs)]
    wst = ops.esmm_stacked_weight(sh, towers)
    own = model.__dict__.setdefault("_train_images", {})
    if own.get("device") != dev:
        own.clear()
        own["device"] = dev
    pairs, tstacks = [], []

    def image(key, w):
        img = own.get(key)
        if img is None:
            img = own[key] = ops.mlp_image(w.shape[0], w.shape[1], dev)
        pairs.append((w, img))
        return img
    for k, (hidden, _) in enumerate(towers):
        tstacks.append([(image(("t", k, l), w), b, w.shape[0], "relu") for l, (w, b) in enumerate(hidden)])
    ops.pack_mlp_weights(pairs, ops._lib.raw_stream(dev))
    p = float(model.dropout_rate)
    seed, slot = 0, None
    if p > 0:
        seed, slot = model.__dict__.setdefault("_dropout", DropoutStreams()).next(dev)
    heads = [(w, b) for _, (w, b) in towers]
    s = ops.esmm_forward_train(model._segments(dense, names, idx), sh, B, tstacks, heads, dev, p, seed, slot)
    s["weights"] = (towers, wst)
    s["dropout"] = (seed, slot)
    return sh, s


class _ESMMTrain(torch.autograd.Function):
    """ESMM forward + backward in train mode: rk_esmm_forward_train (one launch: the gather, the towers with
    dropout, the heads and the chain, every activation kept), then ops.esmm_backward (the fold onto the
    logits, the heads, the towers grouped over the tasks, the stacked layer 0: a fixed number of launches
    whatever K) and the embedding gradients.  Inputs after the fixed arguments: the tables, then every
    tower Linear's (weight, bias) tower-major, the output layers'."""

    @staticmethod
    def forward(ctx, model, dense, names, idx, *params):
        sh, s = _esmm_front(model, dense, names, idx)
        ctx.model, ctx.sh, ctx.s, ctx.names, ctx.idx, ctx.B = model, sh, s, names, idx, dense.shape[0]
        ctx.set_materialize_grads(False)
        return s["probs"], s["logits"]

    @staticmethod
    def backward(ctx, dprob, dlogit):
        model, sh, s, B = ctx.model, ctx.sh, ctx.s, ctx.B
        dev = s["x"].device
        towers, wst = s["weights"]
        if dprob is None and dlogit is None:
            dlogit = torch.zeros(B, sh.K, device=dev, dtype=torch.float32)
        dx, tg = ops.esmm_backward(sh, B, s, wst, towers, float(model.dropout_rate), _grad_out(dlogit, s["logits"]),
                                   _grad_out(dprob, s["probs"]), None, True, dev)
        tables = [model.embeddings[n].weight for n in ctx.names]
        out = list(embedding_grads(tables, ctx.idx, model.num_dense_features, dx, sparse=model.sparse_grad))
        for k in range(sh.K):
            for l in range(len(sh.tu)):
                out += list(tg[k][0][l])
        for k in range(sh.K):
            out += [tg[k][1][0], tg[k][1][1]]
        return (None, None, None, None, *out)


def _esmm_params(model, names):
    lin = model._linears
    params = [model.embeddings[n].weight for n in names]
    for seq in model.towers:
        for l in lin(seq):
            params += [l.weight, l.bias]
    for o in model.tower_outputs:
        params += [o.weight, o.bias]
    return params


# ---------------------------------------------------------------- DIN

def din_units(model):
    """(Linear, Dice or PReLU module, BatchNorm1d or None, dropout p) per fcn unit (din.py:272-284)."""
    units = []
    for m in model.fcn:
        if isinstance(m, torch.nn.Linear):
            units.append([m, None, None, 0.0])
        elif isinstance(m, torch.nn.BatchNorm1d):
            units[-1][2] = m
        elif isinstance(m, torch.nn.Dropout):
            units[-1][3] = float(m.p) if m.training else 0.0
        else:  # Dice, or nn.PReLU with activation='prelu' (din.py:275-279)
            units[-1][1] = m
    for lin, act, bn, _ in units:
        if lin.bias is None or act is None:
            raise NotImplementedError("rankops DIN training expects the reference's Linear + Dice / PReLU units")
        if (not isinstance(act, torch.nn.PReLU) and act.bn.momentum is None) or (bn is not None and bn.momentum is None):
            raise NotImplementedError("rankops DIN training: BatchNorm1d needs a numeric momentum")
    return units


def din_tail_forward(model, x, units, seed, slot):
    """The fcn units Linear -> Dice / PReLU -> BatchNorm1d -> Dropout with batch statistics over the
    row x [B, width], then output_layer + sigmoid (din.py:272-288, the tail DIEN shares); returns
    (per-unit saved tensors, prob, logit)."""
    B, dev = x.shape[0], x.device
    f32 = dict(device=dev, dtype=torch.float32)
    saved = []
    h = x
    for u, (lin, dice, bn, p) in enumerate(units):
        n, K = lin.out_features, lin.in_features
        z = torch.empty(B, n, **f32)
        ops.gemm(False, False, B, n, K, h, h.stride(0), lin.weight, lin.weight.stride(0), z)
        y1 = torch.empty(B, n, **f32)
        m1, s1 = torch.empty(n, **f32), torch.empty(n, **f32)
        if isinstance(dice, torch.nn.PReLU):
            ops.prelu_train_forward(z, lin.bias, dice, y1)
        else:
            ops.dice_train_forward(z, lin.bias, dice, y1, m1, s1,
                                   torch.empty(2 * n, device=dev, dtype=torch.float64))
        y2, m2, s2 = y1, m1, s1
        if bn is not None or p > 0:
            y2 = torch.empty(B, n, **f32)
            m2, s2 = torch.empty(n, **f32), torch.empty(n, **f32)
            ops.bn_act_train_forward(y1, None, bn, False, p, seed + u, slot, y2, m2, s2,
                                     torch.empty(2 * n, device=dev, dtype=torch.float64))
        saved.append((z, y1, m1, s1, y2, m2, s2))
        h = y2
    logit = torch.empty(B, 1, **f32)
    prob = torch.empty(B, 1, **f32)
    ops.mlp_forward(h, [], ops.make_epilogue(head_w=model.output_layer.weight, head_b=model.output_layer.bias,
                                             head_logit=logit, head_prob=prob))
    return saved, prob, logit


def din_tail_backward(model, dprob, dlogit, prob, x, units, saved, seed, slot):
    """Backward of din_tail_forward: rk_logit_head_backward, then the units last to first; returns
    (dL/dx [B, width], per-unit grads [dW, db, dalpha, (dgamma, dbeta)], dw_out, db_out)."""
    B, dev = x.shape[0], x.device
    f32 = dict(device=dev, dtype=torch.float32)
    last = saved[-1][4] if saved else x
    dy = torch.empty_like(last)
    w_out = model.output_layer.weight
    dw_out = torch.empty_like(w_out)
    db_out = torch.empty(1, **f32)
    ops.logit_head_backward(_grad_out(dlogit, prob), _grad_out(dprob, prob), prob, last, None, w_out, dy, None,
                            dw_out, db_out)
    unit_grads = [None] * len(units)
    for u in range(len(units) - 1, -1, -1):
        lin, dice, bn, p = units[u]
        z, y1, m1, s1, y2, m2, s2 = saved[u]
        n, K = lin.out_features, lin.in_features
        h_in = saved[u - 1][4] if u > 0 else x
        dy1 = dy
        dg = dbt = None
        if bn is not None or p > 0:
            dy1 = torch.empty(B, n, **f32)
            if bn is not None:
                dg = torch.empty(n, **f32) if bn.weight is not None else None
                dbt = torch.empty(n, **f32) if bn.bias is not None else None
            ops.bn_act_backward(dy, y1, None, bn, False, p, seed + u, slot, m2, s2,
                                torch.empty(2 * n, device=dev, dtype=torch.float64), dy1, dg, dbt)
        dz = torch.empty(B, n, **f32)
        if isinstance(dice, torch.nn.PReLU):
            dalpha = torch.empty_like(dice.weight)
            ops.prelu_backward(dy1, z, lin.bias, dice, torch.empty(dice.weight.numel(), device=dev,
                                                                   dtype=torch.float64), dz, dalpha)
        else:
            dalpha = torch.empty(n, **f32)
            ops.dice_backward(dy1, z, lin.bias, dice, m1, s1, torch.empty(3 * n, device=dev, dtype=torch.float64),
                              dz, dalpha)
        dW = torch.empty(n, K, **f32)
        db = torch.empty(n, **f32)
        ops.gemm(True, True, n, K, B, dz, dz.stride(0), h_in, h_in.stride(0), dW, row_sums=db)
        dx = torch.empty(B, K, **f32)
        ops.gemm(False, True, B, K, n, dz, dz.stride(0), lin.weight, lin.weight.stride(0), dx)
        unit_grads[u] = [dW, db, dalpha] + ([t for t in (dg, dbt) if t is not None] if bn is not None else [])
        dy = dx
    return dy, unit_grads, dw_out, db_out


class _DINTrain(torch.autograd.Function):
    """DIN forward + backward in train mode (din.py:294-323): gather, din_attention (att_net's
    layers as GEMMs on rk_linear with the activations kept for the backward, the weights drawn per
    call like the reference and not trained), fcn units Linear -> Dice / PReLU -> BatchNorm1d -> Dropout
    with batch statistics, output_layer + sigmoid, and the mini-batch-aware l2 term.
    Inputs after the fixed arguments are the parameters in `_din_params` order."""

    @staticmethod
    def forward(ctx, model, pl, att, emb_plan, *params):
        B, dev, H = pl["B"], pl["dev"], pl["H"]
        q_col, att_col, width, cat_col0 = pl["q_col"], pl["att_col"], pl["width"], pl["cat_col0"]
        seq, seq_len = pl["seq"], pl["seq_len"]
        T = seq.shape[1]
        f32 = dict(device=dev, dtype=torch.float32)
        x = torch.empty(B, width, **f32)
        ops.concat_gather(pl["segs"], B, x)  # [dense | category | target]; the attention columns below
        w1, b1, w2, b2, w3, b3 = att
        keys = torch.empty(B, T, H, **f32)
        cross = torch.empty(B * T, 4 * H, **f32)
        ops.din_att_cross(x, q_col, model.embeddings[pl["seq_key"]].weight, seq, T, H, keys, cross)
        a1 = torch.empty(B * T, w1.shape[0], **f32)
        ops.linear(cross, w1, a1, epilogue=ops.make_epilogue(bias=b1, act="relu"))
        a2 = torch.empty(B * T, w2.shape[0], **f32)
        ops.linear(a1, w2, a2, epilogue=ops.make_epilogue(bias=b2, act="relu"))
        del cross
        wts = torch.empty(B, T, **f32)
        ops.din_att_pool_forward(a2, w3.reshape(-1), b3, keys, seq_len, T, H, model.use_softmax, wts, x, att_col)
        units = din_units(model)
        seed, slot = model._dropout.next(dev)
        saved, prob, logit = din_tail_forward(model, x, units, seed, slot)
        l2 = torch.zeros((), **f32)
        if pl["want_l2"]:
            ops.row_l2norm_mean(x, cat_col0, width - cat_col0, float(model.l2_lambda), l2)
        ctx.model, ctx.pl, ctx.units, ctx.seed, ctx.emb_plan = model, pl, units, seed, emb_plan
        ctx.save_for_backward(x, keys, a1, a2, wts, prob, slot, w1, w2, w3, *[t for s in saved for t in s])
        return prob, logit, l2

    @staticmethod
    def backward(ctx, dprob, dlogit, dl2):
        model, pl, units = ctx.model, ctx.pl, ctx.units
        x, keys, a1, a2, wts, prob, slot, w1, w2, w3, *flat = ctx.saved_tensors
        saved = [tuple(flat[7 * u:7 * u + 7]) for u in range(len(units))]
        B, dev, H = pl["B"], pl["dev"], pl["H"]
        T = keys.shape[1]
        f32 = dict(device=dev, dtype=torch.float32)
        dxr, unit_grads, dw_out, db_out = din_tail_backward(model, dprob, dlogit, prob, x, units, saved, ctx.seed, slot)
        # dxr = dL/d[dense | category | target | attention]
        if pl["want_l2"] and dl2 is not None:
            ops.row_l2norm_backward(x, pl["cat_col0"], pl["width"] - pl["cat_col0"], float(model.l2_lambda) / B,
                                    dl2.to(torch.float32).reshape(1).contiguous(), dxr)
        # din_attention backward: weighted sum and scores, then att_net (its weights are not trained)
        M = B * T
        dkeys = torch.empty(B, T, H, **f32)
        da2 = torch.empty(M, a2.shape[1], **f32)
        ops.din_att_pool_backward(dxr, pl["att_col"], wts, keys, a2, w3.reshape(-1), pl["seq_len"], T, H,
                                  model.use_softmax, dkeys, da2)
        da1 = torch.empty(M, a1.shape[1], **f32)
        ops.gemm(False, True, M, a1.shape[1], a2.shape[1], da2, da2.stride(0), w2, w2.stride(0), da1)
        dcross = torch.empty(M, 4 * H, **f32)
        ops.gemm(False, True, M, 4 * H, a1.shape[1], da1, da1.stride(0), w1, w1.stride(0), dcross, A_mask=a1)
        ops.din_cross_fold(dcross, x, pl["q_col"], keys, T, H, dkeys, dxr)
        del dcross
        # nn.Embedding gradients: one zeroed buffer per distinct table, every lookup scattered into it
        weights, looks = ctx.emb_plan
        flat = [t for g in unit_grads for t in g]
        if model.sparse_grad:  # the shared feedid table: target lookup + every history position
            sources = [[] for _ in weights]
            for k, i, col in looks:
                sources[k].append((i, dxr, col))
            sources[pl["seq_slot"]].append((pl["seq"].reshape(-1), dkeys.view(M, H), 0))
            return (None, None, None, None, *sparse_embedding_grads(weights, sources), *flat, dw_out, db_out)
        grads = zero_grads(weights, dev)
        segs = [ops.table_segment(grads[k], i, col) for k, i, col in looks]
        ops.embedding_backward(segs, B, dxr)
        # History keys past seq_len get exactly zero gradient (their attention weight is 0 and so is
        # their score's gradient, din.py:61-84), so the padded positions that all map to row 0 add
        # nothing and the zero-skipping atomic scatter stays contention-free (the sorted
        # segment-reduce, whose radix sort alone costs ~85 us here, is only needed where padded
        # positions carry gradient: BST's sum pooling; the length-0 softmax case, where all T
        # weights are 1/T, is still exact, only slower).
        ops.embedding_backward([ops.table_segment(grads[pl["seq_slot"]], pl["seq"].reshape(-1), 0)], M,
                               dkeys.view(M, H))
        return (None, None, None, None, *grads, *flat, dw_out, db_out)


def _din_params(model, units):
    out = []
    for lin, act, bn, _ in units:
        out += [lin.weight, lin.bias, act.weight if isinstance(act, torch.nn.PReLU) else act.alpha]
        if bn is not None:
            out += [t for t in (bn.weight, bn.bias) if t is not None]
    return out + [model.output_layer.weight, model.output_layer.bias]


def din_train_forward(model, pl, att):
    """DIN train-mode forward with autograd (rankops.DIN.forward in model.train())."""
    units = din_units(model)
    # distinct embedding tables in first-use order and the (table slot, index, column) lookups
    weights, looks = [], []

    def slot_of(w):
        for k, t in enumerate(weights):
            if t is w:
                return k
        weights.append(w)
        return len(weights) - 1

    for w, idx, col in pl["lookups"]:
        looks.append((slot_of(w), idx, col))
    pl = dict(pl, seq_slot=slot_of(model.embeddings[pl["seq_key"]].weight))
    return _DINTrain.apply(model, pl, att, (weights, looks), *weights, *_din_params(model, units))


# ---------------------------------------------------------------- DIEN

def dien_tail_forward(model, pl, x, att, hs=None, ss=None):
    """DIEN's train-mode forward over the gathered row x: the interest state into its last nh columns
    (the train kernel when hs / ss are given, which keeps them for the backward), then DIN's tail."""
    from .dien import _cell
    B, dev, H, nh, width = pl["B"], pl["dev"], pl["H"], model.gru_output_units, pl["width"]
    T = pl["seq"].shape[1]
    table = model.embeddings["feedid"].weight
    args = (ops._lib.fptr(x, pl["q_col"]), width, table, pl["seq"], pl["seq_len"], T, H, nh,
            _cell(model.custom_gru_type), model.interest_weights(), ops._lib.fptr(x, pl["state_col"]), width, att)
    if hs is None:
        ops.dien_interest(*args, B, dev)
    else:
        ops.dien_interest_train(*args, hs, ss, B, dev)
    units = din_units(model)
    seed, slot = model._dropout.next(dev)
    saved, prob, logit = din_tail_forward(model, x, units, seed, slot)
    return units, seed, slot, saved, prob, logit


def dien_aux_forward(model, pl, hs):
    """The auxiliary loss of the kept extractor states (rk_dien_aux_loss over the feedid table, the
    history ids and pl["neg_seq"]): a 0-dim tensor."""
    B, dev, H, nh = pl["B"], pl["dev"], pl["H"], model.gru_output_units
    T = pl["seq"].shape[1]
    per_sample = torch.empty(B, device=dev, dtype=torch.float32)
    mean = torch.empty(1, device=dev, dtype=torch.float32)
    ops.dien_aux_loss(hs, model.embeddings["feedid"].weight, pl["seq"], None, pl["neg_seq"], pl["seq_len"], T,
                      model.negative_sample_number, H, nh, model.aux_project_matrix, per_sample, mean, B, dev)
    return mean.reshape(())


class _DIENTrain(torch.autograd.Function):
    """DIEN forward + backward in train mode (dien.py:166-254,314-334): rk_concat_gather, the train
    interest forward (GRU, attention, AGRU / AUGRU, states kept), DIN's tail with batch statistics
    and Dropout; backward: head, units, rk_dien_interest_backward reading d(state) from the row
    gradient's state columns and adding dquery into its target columns, then the embedding scatters.
    Inputs after the fixed arguments: the distinct tables, the nine interest weights, `_din_params`,
    and with the auxiliary loss (pl["neg_seq"] set) aux_project_matrix last.  Then the forward also
    returns the auxiliary loss of the kept states (dien.py:256-300), and the backward, if that loss
    received a gradient, runs rk_dien_aux_loss_backward first: its d_hs enters the extractor's chain
    and its dkeys is added to (rk_dien_interest_backward_aux), and its dneg is one more scatter
    into the feedid table's gradient."""

    @staticmethod
    def forward(ctx, model, pl, emb_plan, *params):
        B, dev, nh, width = pl["B"], pl["dev"], model.gru_output_units, pl["width"]
        T = pl["seq"].shape[1]
        f32 = dict(device=dev, dtype=torch.float32)
        x = torch.empty(B, width, **f32)
        ops.concat_gather(pl["segs"], B, x)  # [dense | category | target | .]
        att = torch.empty(B, T, **f32)
        hs, ss = torch.empty(B, T, nh, **f32), torch.empty(B, T, nh, **f32)
        units, seed, slot, saved, prob, logit = dien_tail_forward(model, pl, x, att, hs, ss)
        ctx.model, ctx.pl, ctx.units, ctx.seed, ctx.emb_plan = model, pl, units, seed, emb_plan
        ctx.save_for_backward(x, att, hs, ss, prob, slot, *[t for s in saved for t in s])
        ctx.mark_non_differentiable(att)
        if "neg_seq" not in pl:
            return prob, logit, att
        ctx.set_materialize_grads(False)  # an unused aux loss arrives as None and costs nothing
        return prob, logit, att, dien_aux_forward(model, pl, hs)

    @staticmethod
    def backward(ctx, dprob, dlogit, _datt, daux=None):
        from .dien import _cell
        model, pl, units = ctx.model, ctx.pl, ctx.units
        x, att, hs, ss, prob, slot, *flat = ctx.saved_tensors
        saved = [tuple(flat[7 * u:7 * u + 7]) for u in range(len(units))]
        B, dev, H, nh, width = pl["B"], pl["dev"], pl["H"], model.gru_output_units, pl["width"]
        seq = pl["seq"]
        T = seq.shape[1]
        if dprob is None:  # only the auxiliary loss's gradients are left unmaterialised
            dprob = torch.zeros_like(prob)
        if dlogit is None:
            dlogit = torch.zeros_like(prob)
        dxr, unit_grads, dw_out, db_out = din_tail_backward(model, dprob, dlogit, prob, x, units, saved, ctx.seed, slot)
        # dxr = dL/d[dense | category | target | state]: d(state) is read in place, dquery added in place
        weights, looks = ctx.emb_plan
        table = model.embeddings["feedid"].weight
        aux = "neg_seq" in pl
        d_hs = dneg = neg_ids = daux_w = None
        if aux and daux is not None:  # the auxiliary loss first: it writes dkeys in full, the recurrence adds
            neg_ids = torch.empty_like(pl["neg_seq"])
            d_hs, dkeys, dneg, daux_w = ops.dien_aux_loss_backward(
                hs, table, seq, None, pl["neg_seq"], pl["seq_len"], T, model.negative_sample_number, H, nh,
                model.aux_project_matrix, daux.to(torch.float32).reshape(1).contiguous(), B, dev, None, neg_ids)
        else:
            dkeys = torch.empty(B, T, H, device=dev, dtype=torch.float32)
        ids = torch.empty_like(seq)  # the history ids with 0 past the length (poisoned tails never scatter)
        wgrads = ops.dien_interest_backward(ops._lib.fptr(x, pl["q_col"]), width, table, seq, 0, pl["seq_len"], T, H,
                                            nh, _cell(model.custom_gru_type), model.interest_weights(), hs, ss, att,
                                            ops._lib.fptr(dxr, pl["state_col"]), width,
                                            ops._lib.fptr(dxr, pl["q_col"]), width, True, dkeys, B, dev, ids,
                                            d_hs=d_hs, accumulate_dkeys=d_hs is not None)
        # one zeroed buffer per distinct table; feedid takes the target lookup and the history scatter
        # (key rows past the length are exact zeros: the zero-skipping scatter stays contention-free)
        if model.sparse_grad:  # feedid: target lookup + history (+ the auxiliary loss's negatives)
            sources = [[] for _ in weights]
            for k, i, col in looks:
                sources[k].append((i, dxr, col))
            sources[pl["seq_slot"]].append((ids.reshape(-1), dkeys.view(B * T, H), 0))
            if dneg is not None and dneg.numel():
                sources[pl["seq_slot"]].append((neg_ids.reshape(-1), dneg.view(neg_ids.numel(), H), 0))
            return (None, None, None, *sparse_embedding_grads(weights, sources), *wgrads,
                    *[t for g in unit_grads for t in g], dw_out, db_out, *([daux_w] if aux else []))
        grads = zero_grads(weights, dev)
        ops.embedding_backward([ops.table_segment(grads[k], i, col) for k, i, col in looks], B, dxr)
        ops.embedding_backward([ops.table_segment(grads[pl["seq_slot"]], ids.reshape(-1), 0)], B * T,
                               dkeys.view(B * T, H))
        if dneg is not None and dneg.numel():
            n = neg_ids.numel()
            ops.embedding_backward([ops.table_segment(grads[pl["seq_slot"]], neg_ids.reshape(-1), 0)], n,
                                   dneg.view(n, H))
        return (None, None, None, *grads, *wgrads, *[t for g in unit_grads for t in g], dw_out, db_out,
                *([daux_w] if aux else []))


def dien_train_forward(model, pl, grad: bool):
    """DIEN train-mode forward (rankops.DIEN.forward in model.train()): (prob, logit, attention),
    and the auxiliary loss when pl carries the negatives, attached to _DIENTrain when `grad`;
    otherwise the same launches with nothing kept."""
    aux = "neg_seq" in pl
    if not grad:
        B, dev = pl["B"], pl["dev"]
        T, nh = pl["seq"].shape[1], model.gru_output_units
        f32 = dict(device=dev, dtype=torch.float32)
        x = torch.empty(B, pl["width"], **f32)
        ops.concat_gather(pl["segs"], B, x)
        att = torch.empty(B, T, **f32)
        if not aux:
            _, _, _, _, prob, logit = dien_tail_forward(model, pl, x, att)
            return prob, logit, att
        hs = torch.empty(B, T, nh, **f32)  # the train forward kernel, for the states the loss reads
        _, _, _, _, prob, logit = dien_tail_forward(model, pl, x, att, hs, torch.empty(B, T, nh, **f32))
        return prob, logit, att, dien_aux_forward(model, pl, hs)
    units = din_units(model)
    weights, looks = [], []

    def slot_of(w):
        for k, t in enumerate(weights):
            if t is w:
                return k
        weights.append(w)
        return len(weights) - 1

    for w, idx, col in pl["lookups"]:
        looks.append((slot_of(w), idx, col))
    pl = dict(pl, seq_slot=slot_of(model.embeddings["feedid"].weight))
    return _DIENTrain.apply(model, pl, (weights, looks), *weights, *model.interest_weights(),
                            *_din_params(model, units), *([model.aux_project_matrix] if aux else []))


# ---------------------------------------------------------------- AFM

class _AFMTrain(torch.autograd.Function):
    """AFM forward + backward (afm.py:92-119; no train/eval difference in the module).  Inputs
    after the fixed arguments: dense_layer.{weight,bias}, the field embeddings, attention.0.{weight,
    bias}, attention.2.{weight,bias}, p.{weight,bias}."""

    @staticmethod
    def forward(ctx, model, dense, idx, *params):
        F, D = model.num_fields, model.embedding_dim
        wd, bd = params[0], params[1]
        tables = params[2:2 + F]
        w1, b1, w2, b2, wp, bp = params[2 + F:]
        B, dev = dense.shape[0], dense.device
        P = F * (F - 1) // 2
        f32 = dict(device=dev, dtype=torch.float32)
        emb = torch.empty(B, F * D, **f32)
        pairs = torch.empty(B * P, D, **f32)
        ops.afm_pairs([ops.table_segment(t, i, 0) for t, i in zip(tables, idx)], D, B, emb, pairs)
        a1 = torch.empty(B * P, w1.shape[0], **f32)
        ops.linear(pairs, w1, a1, epilogue=ops.make_epilogue(bias=b1, act="relu"))
        weights = torch.empty(B, P, **f32)
        ws = torch.empty(B, D, **f32)
        logit = torch.empty(B, 1, **f32)
        pred = torch.empty(B, 1, **f32)
        ops.afm_pool_forward(a1, w2.reshape(-1), b2, pairs, P, D, dense, wd.reshape(-1), bd, wp.reshape(-1), bp,
                             weights, ws, logit, pred)
        ctx.model, ctx.idx = model, idx
        ctx.save_for_backward(dense, emb, pairs, a1, weights, ws, pred, w1, w2, wp, *tables)
        return pred, logit

    @staticmethod
    def backward(ctx, dpred, dlogit):
        model, idx = ctx.model, ctx.idx
        dense, emb, pairs, a1, weights, ws, pred, w1, w2, wp, *tables = ctx.saved_tensors
        F, D = model.num_fields, model.embedding_dim
        B, dev = dense.shape[0], dense.device
        P, A, nd = F * (F - 1) // 2, w1.shape[0], dense.shape[1]
        f32 = dict(device=dev, dtype=torch.float32)
        d_pairs = torch.empty(B * P, D, **f32)
        da1 = torch.empty(B * P, A, **f32)
        acc = torch.empty(nd + 1 + D + 1 + A + 1, **f32)
        ops.afm_pool_backward(_grad_out(dpred, pred) if dpred is not None else None,
                              _grad_out(dlogit, pred) if dlogit is not None else None, pred, weights, ws, pairs, a1,
                              w2.reshape(-1), wp.reshape(-1), dense, P, D, d_pairs, da1, acc)
        dW1 = torch.empty_like(w1)
        db1 = torch.empty(A, **f32)
        M = B * P
        ops.gemm(True, True, A, D, M, da1, A, pairs, D, dW1, row_sums=db1)
        ops.gemm(False, True, M, D, A, da1, A, w1, D, d_pairs, accumulate=True)
        d_emb = torch.empty(B, F * D, **f32)
        ops.afm_pair_fold(d_pairs, emb, F, D, d_emb)
        g_emb = embedding_grads(list(tables), idx, 0, d_emb, sparse=model.sparse_grad)
        o = 0
        dwd, dbd = acc[o:o + nd].view(1, nd), acc[o + nd:o + nd + 1]
        o += nd + 1
        dwp, dbp = acc[o:o + D].view(1, D), acc[o + D:o + D + 1]
        o += D + 1
        dw2, db2 = acc[o:o + A].view(1, A), acc[o + A:o + A + 1]
        return (None, None, None, dwd, dbd, *g_emb, dW1, db1, dw2, db2, dwp, dbp)


def afm_train_forward(model, dense, idx):
    att1, att2 = model.attention[0], model.attention[2]
    params = ([model.dense_layer.weight, model.dense_layer.bias]
              + [model.embeddings[c].weight for c in model.category_features]
              + [att1.weight, att1.bias, att2.weight, att2.bias, model.p.weight, model.p.bias])
    if any(t is None for t in params):
        raise NotImplementedError("rankops AFM training expects the reference's biased Linear layers")
    return _AFMTrain.apply(model, dense, idx, *params)


# ---------------------------------------------------------------- BST

def bst_units(model):
    """([Linear, BatchNorm1d or None, 'leaky', dropout p, slope] per dnn unit, last Linear)
    (bst.py:203-213)."""
    mods = list(model.dnn)
    units = []
    for m in mods[:-1]:
        if isinstance(m, torch.nn.Linear):
            units.append([m, None, "none", 0.0, 0.0])
        elif isinstance(m, torch.nn.BatchNorm1d):
            if m.momentum is None:
                raise NotImplementedError("rankops BST training: BatchNorm1d needs a numeric momentum")
            units[-1][1] = m
        elif isinstance(m, torch.nn.LeakyReLU):
            units[-1][2], units[-1][4] = "leaky", float(m.negative_slope)
        elif isinstance(m, torch.nn.Dropout):
            units[-1][3] = float(m.p) if m.training else 0.0
        else:
            raise NotImplementedError(f"rankops BST training: unsupported dnn layer {type(m).__name__}")
    return units, mods[-1]


def _block_params(blk):
    return [blk.position_embedding.weight, blk.w_q.weight, blk.w_q.bias, blk.w_k.weight, blk.w_k.bias,
            blk.w_v.weight, blk.w_v.bias, blk.w_o.weight, blk.w_o.bias, blk.norm1.weight, blk.norm1.bias,
            blk.norm2.weight, blk.norm2.bias, blk.ffn[0].weight, blk.ffn[0].bias, blk.ffn[3].weight, blk.ffn[3].bias]


def bst_dropout_seed(seed, block, site):
    """Dropout stream seed of transformer block `block`, site 0 (w_o output), 1 (inside the FFN),
    2 (FFN output); the dnn units use seed + unit."""
    return seed + 100 + 3 * block + site


def _lin_grads(dy, x, w, need_dx=True, dx=None, accumulate=False):
    """y = x W^T + b backward with dy row stride dy.stride(0): (dW, db[, dx])."""
    M, N = dy.shape[0], w.shape[0]
    K = w.shape[1]
    dW = torch.empty(N, K, device=dy.device, dtype=torch.float32)
    db = torch.empty(N, device=dy.device, dtype=torch.float32)
    ops.gemm(True, True, N, K, M, dy, dy.stride(0), x, x.stride(0), dW, row_sums=db)
    if need_dx:
        if dx is None:
            dx = torch.empty(M, K, device=dy.device, dtype=torch.float32)
        ops.gemm(False, True, M, K, N, dy, dy.stride(0), w, w.stride(0), dx, accumulate=accumulate)
    return dW, db, dx


_POSITION_IDS = {}


def _position_ids(B, T, device):
    """The position lookups of a [B, T] batch, 0..T-1 per sample, flattened; kept per (B, T, device)
    (a tensor made while a graph is being captured belongs to that graph and is not kept)."""
    key = (B, T, device)
    ids = _POSITION_IDS.get(key)
    if ids is None:
        ids = torch.arange(T, device=device).repeat(B)
        if not torch.cuda.is_current_stream_capturing():
            if len(_POSITION_IDS) >= 64:
                _POSITION_IDS.clear()
            _POSITION_IDS[key] = ids
    return ids


class _BSTTrain(torch.autograd.Function):
    """BSTModel forward + backward in train mode (bst.py:216-247 with BSTTransformer.forward
    bst.py:66-91): Dropout in every block (w_o output, inside and after the FFN) and in the dnn,
    BatchNorm1d with batch statistics.  Inputs after the fixed arguments: the distinct embedding
    tables of `plan`, then per block `_block_params`, then the dnn unit parameters and the last
    Linear."""

    @staticmethod
    def forward(ctx, model, plan, *params):
        seq, seq_len, B, T, width, col = plan["seq"], plan["seq_len"], plan["B"], plan["T"], plan["width"], plan["col"]
        dev, d = seq.device, model.d_model
        M = B * T
        f32 = dict(device=dev, dtype=torch.float32)
        row = torch.empty(B, width, **f32)
        ops.concat_gather(plan["segs"], B, row)
        feed = model.embeddings["feedid"].weight
        x = torch.empty(M, d, **f32)
        seed, slot = model._dropout.next(dev)
        saves = []
        for i, blk in enumerate(model.transformer_blocks):
            p_o, p_f = float(blk.dropout.p) if blk.training else 0.0, float(blk.ffn[2].p) if blk.training else 0.0
            h = blk.nhead
            xp = torch.empty(M, d, **f32)
            pos = blk.position_embedding.weight
            if i > 0 or not ops.bst_gather_pos(feed, seq.reshape(-1), T, pos, x, xp):
                if i == 0:
                    ops.concat_gather([ops.table_segment(feed, seq.view(-1), 0)], M, x)
                ops.bst_add_pos(x, pos, T, xp)
            qkv = torch.empty(M, 3 * d, **f32)
            ops.linear(xp, blk.w_q.weight, None, y_ptr=qkv.data_ptr(), ldy=3 * d,
                       epilogue=ops.make_epilogue(bias=blk.w_q.bias))
            ops.linear(xp, blk.w_k.weight, None, y_ptr=ops._lib.fptr(qkv, d), ldy=3 * d,
                       epilogue=ops.make_epilogue(bias=blk.w_k.bias))
            ops.linear(x, blk.w_v.weight, None, y_ptr=ops._lib.fptr(qkv, 2 * d), ldy=3 * d,
                       epilogue=ops.make_epilogue(bias=blk.w_v.bias))
            cx = torch.empty(M, d, **f32)
            # P is kept for the backward (recomputing it there measured slower at configs[3]: backward
            # 185 -> 242 us against forward 114 -> 108 us)
            probs = torch.empty(B * h * T * T, **f32)
            ops.bst_attn_train_forward(qkv, B, T, d, h, seq_len, probs, cx)
            r1, out1 = torch.empty(M, d, **f32), torch.empty(M, d, **f32)
            m1, s1 = torch.empty(M, **f32), torch.empty(M, **f32)
            # out1 = LN1(xp + dropout(w_o(cx))): one launch when the shape allows
            if not (FUSED_LN and ops.linear_res_dropout_ln(cx, blk.w_o.weight, blk.w_o.bias, xp, p_o,
                                                           bst_dropout_seed(seed, i, 0), slot, blk.norm1, r1, out1,
                                                           m1, s1)):
                o = torch.empty(M, d, **f32)
                ops.linear(cx, blk.w_o.weight, o, epilogue=ops.make_epilogue(bias=blk.w_o.bias))
                ops.bst_res_dropout_ln_forward(xp, o, p_o, bst_dropout_seed(seed, i, 0), slot, blk.norm1, r1, out1, m1,
                                               s1)
                del o
            f1 = torch.empty(M, d, **f32)
            ops.linear(out1, blk.ffn[0].weight, f1, epilogue=ops.make_epilogue(bias=blk.ffn[0].bias))
            a = torch.empty(M, d, **f32)
            ops.bst_leaky_dropout(None, f1, blk.ffn[1].negative_slope, p_f, bst_dropout_seed(seed, i, 1), slot, False, a)
            r2, out = torch.empty(M, d, **f32), torch.empty(M, d, **f32)
            m2, s2 = torch.empty(M, **f32), torch.empty(M, **f32)
            if not (FUSED_LN and ops.linear_res_dropout_ln(a, blk.ffn[3].weight, blk.ffn[3].bias, out1, p_o,
                                                           bst_dropout_seed(seed, i, 2), slot, blk.norm2, r2, out,
                                                           m2, s2)):
                f2 = torch.empty(M, d, **f32)
                ops.linear(a, blk.ffn[3].weight, f2, epilogue=ops.make_epilogue(bias=blk.ffn[3].bias))
                ops.bst_res_dropout_ln_forward(out1, f2, p_o, bst_dropout_seed(seed, i, 2), slot, blk.norm2, r2, out,
                                               m2, s2)
            saves.append((x, xp, qkv, probs, cx, r1, out1, m1, s1, f1, a, r2, m2, s2))
            x = out
        mean_pool = model.pooling_method != "sum"
        if not saves:  # no blocks: transformer_output = seq_emb (bst.py:229), pooled over all T positions
            ops.concat_gather([ops.table_segment(feed, seq.view(-1), 0)], M, x)
        ops.bst_pool(x, B, T, seq_len, mean_pool, row, col)
        units, last = bst_units(model)
        saved = deep_stack_forward(row, units, seed, slot)
        hid = saved[-1][1] if saved else row
        logit = torch.empty(B, 1, **f32)
        prob = torch.empty(B, 1, **f32)
        ops.mlp_forward(hid, [], ops.make_epilogue(head_w=last.weight, head_b=last.bias, head_logit=logit,
                                                   head_prob=prob))
        ctx.model, ctx.plan, ctx.units, ctx.seed, ctx.nsave = model, plan, units, seed, len(saves)
        ctx.save_for_backward(row, prob, slot, *[t for sv in saves for t in sv], *[t for sv in saved for t in sv])
        return prob, logit

    @staticmethod
    def backward(ctx, dprob, dlogit):
        model, plan, units, seed = ctx.model, ctx.plan, ctx.units, ctx.seed
        row, prob, slot, *flat = ctx.saved_tensors
        nb = ctx.nsave
        saves = [tuple(flat[14 * i:14 * i + 14]) for i in range(nb)]
        flat = flat[14 * nb:]
        saved = [tuple(flat[4 * u:4 * u + 4]) for u in range(len(units))]
        seq, seq_len, B, T, col = plan["seq"], plan["seq_len"], plan["B"], plan["T"], plan["col"]
        dev, d = row.device, model.d_model
        M = B * T
        f32 = dict(device=dev, dtype=torch.float32)
        _, last = bst_units(model)
        hid = saved[-1][1] if saved else row
        dh = torch.empty_like(hid)
        dw_last = torch.empty_like(last.weight)
        db_last = torch.empty(1, **f32)
        ops.logit_head_backward(_grad_out(dlogit, prob), _grad_out(dprob, prob), prob, hid, None, last.weight, dh,
                                None, dw_last, db_last)
        d_row, unit_grads = deep_stack_backward(dh, row, units, saved, seed, slot)
        mean_pool = model.pooling_method != "sum"
        dx = None  # the last block's LN2 backward reads the pooling gradient d_row directly
        tables, looks = plan["tables"], plan["looks"]
        tgrads = None if model.sparse_grad else zero_grads(tables, dev)
        block_grads = [None] * nb
        pos_looks = []  # sparse_grad: (position table, its value rows) per block, last block first
        for i in range(nb - 1, -1, -1):
            blk = model.transformer_blocks[i]
            x, xp, qkv, probs, cx, r1, out1, m1, s1, f1, a, r2, m2, s2 = saves[i]
            p_o, p_f = float(blk.dropout.p) if blk.training else 0.0, float(blk.ffn[2].p) if blk.training else 0.0
            # out = LN2(out1 + dropout(f2))
            d_out1 = torch.empty(M, d, **f32)
            df2 = torch.empty(M, d, **f32)
            dg2, dbe2 = torch.empty(d, **f32), torch.empty(d, **f32)
            if dx is None and not ops.bst_pool_ln_backward(d_row, col, T, seq_len, mean_pool, r2, m2, s2, blk.norm2,
                                                           p_o, bst_dropout_seed(seed, i, 2), slot, d_out1, df2, dg2,
                                                           dbe2):
                dx = torch.empty(M, d, **f32)
                ops.bst_pool_backward(d_row, col, B, T, d, seq_len, mean_pool, dx)
            if dx is not None:
                ops.bst_ln_backward(dx, r2, m2, s2, blk.norm2, p_o, bst_dropout_seed(seed, i, 2), slot, d_out1, df2,
                                    dg2, dbe2)
            dW2, db2, da = _lin_grads(df2, a, blk.ffn[3].weight)
            df1 = torch.empty(M, d, **f32)
            ops.bst_leaky_dropout(da, f1, blk.ffn[1].negative_slope, p_f, bst_dropout_seed(seed, i, 1), slot, True, df1)
            dW1, db1, _ = _lin_grads(df1, out1, blk.ffn[0].weight, dx=d_out1, accumulate=True)
            # out1 = LN1(xp + dropout(o))
            dxp = torch.empty(M, d, **f32)
            do = torch.empty(M, d, **f32)
            dg1, dbe1 = torch.empty(d, **f32), torch.empty(d, **f32)
            ops.bst_ln_backward(d_out1, r1, m1, s1, blk.norm1, p_o, bst_dropout_seed(seed, i, 0), slot, dxp, do, dg1,
                                dbe1)
            dWo, dbo, dcx = _lin_grads(do, cx, blk.w_o.weight)
            dqkv = torch.empty(M, 3 * d, **f32)
            ops.bst_attn_train_backward(qkv, probs, dcx, B, T, d, blk.nhead, dqkv)
            dQ, dK, dV = dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:]
            dWq, dbq, _ = _lin_grads(dQ, xp, blk.w_q.weight, dx=dxp, accumulate=True)
            dWk, dbk, _ = _lin_grads(dK, xp, blk.w_k.weight, dx=dxp, accumulate=True)
            # position embedding: every row m adds into pos[m % T]
            # keys/queries carry x + pos, values carry x: dL/dx = dL/dxp + dV Wv
            if model.sparse_grad:
                # the position table's value rows are dL/dxp itself (the lookups of positions 0..T-1
                # per sample): dxp stays as it is until the one packing launch at the end, and dV Wv
                # goes to a buffer of its own
                gpos = None
                pos_looks.append((blk.position_embedding.weight, dxp))
                dWv, dbv, dxv = _lin_grads(dV, x, blk.w_v.weight)
                dx = (dxp, dxv) if i == 0 else torch.add(dxp, dxv)
            else:
                gpos = torch.zeros_like(blk.position_embedding.weight)
                ops.bst_pos_backward(dxp, B, T, gpos)
                dWv, dbv, _ = _lin_grads(dV, x, blk.w_v.weight, dx=dxp, accumulate=True)
                dx = dxp
            block_grads[i] = [gpos, dWq, dbq, dWk, dbk, dWv, dbv, dWo, dbo, dg1, dbe1, dg2, dbe2, dW1, db1, dW2, db2]
        if nb == 0:  # no blocks: the pooling gradient goes straight to the gathered sequence rows
            dx = torch.empty(M, d, **f32)
            ops.bst_pool_backward(d_row, col, B, T, d, seq_len, mean_pool, dx)
        # embedding tables: the category lookups from the dnn input row, the behaviour sequence from dx
        flat_units = [t for g in unit_grads for t in g if t is not None]
        if model.sparse_grad:  # padded positions stay in the list with the gradient sum pooling gives them
            sources = [[] for _ in tables]
            for k, idx, c in looks:
                sources[k].append((idx, d_row, c))
            # block 0's dL/dx arrives as its two summands (dL/dxp, dV Wv), added while packing
            sources[plan["feed_slot"]].append((seq.reshape(-1), *((dx[0], 0, dx[1]) if nb else (dx, 0))))
            pos_ids = _position_ids(B, T, dev)
            grads = sparse_embedding_grads(list(tables) + [w for w, _ in pos_looks],
                                           sources + [[(pos_ids, vals, 0)] for _, vals in pos_looks])
            for i, g in zip(range(nb - 1, -1, -1), grads[len(tables):]):
                block_grads[i][0] = g
            return (None, None, *grads[:len(tables)], *[t for g in block_grads for t in g], *flat_units, dw_last,
                    db_last)
        segs = [ops.table_segment(tgrads[k], idx, c) for k, idx, c in looks]
        if segs:
            ops.embedding_backward(segs, B, d_row)
        # padded positions all map to row 0 and carry non-zero gradients (sum pooling): their runs are
        # pre-summed per sample (rk_embedding_backward_seq), else the sorted segment-reduce
        if not ops.embedding_backward_seq(tgrads[plan["feed_slot"]], seq, dx):
            ops.embedding_backward_sorted(ops.table_segment(tgrads[plan["feed_slot"]], seq.view(-1), 0), M, dx)
        return (None, None, *tgrads, *[t for g in block_grads for t in g], *flat_units, dw_last, db_last)


def bst_train_forward(model, dense, category, seq, seq_len):
    """BSTModel train-mode forward with autograd (rankops.BSTModel.forward in model.train())."""
    B, T = seq.shape
    d = model.d_model
    for blk in model.transformer_blocks:
        if T > 64 or d // blk.nhead > 64 or d % blk.nhead or d > 256:
            raise NotImplementedError("rankops BST training: T <= 64, d_model <= 256, d_model / nhead <= 64")
    segs = [ops.dense_segment(dense, model.num_dense_features, 0)]
    col = model.num_dense_features
    tables, looks = [], []

    def slot_of(w):
        for k, t in enumerate(tables):
            if t is w:
                return k
        tables.append(w)
        return len(tables) - 1

    for name, emb in model.embeddings.items():
        if name in category:
            idx = ops.as_index(category[name], f"category[{name!r}]")
            segs.append(ops.table_segment(emb.weight, idx, col))
            looks.append((slot_of(emb.weight), idx, col))
            col += emb.embedding_dim
    feed_slot = slot_of(model.embeddings["feedid"].weight)
    plan = dict(seq=seq, seq_len=seq_len, B=B, T=T, width=col + d, col=col, segs=segs, tables=tables, looks=looks,
                feed_slot=feed_slot)
    units, last = bst_units(model)
    params = (tables + [t for blk in model.transformer_blocks for t in _block_params(blk)] + _unit_params(units)
              + [last.weight, last.bias])
    return _BSTTrain.apply(model, plan, *params)


# ---------------------------------------------------------------- FwFM

class _FwFMTrain(torch.autograd.Function):
    """FwFM forward (rk_fwfm_forward, fwfm.py:114-139; no train/eval difference) + backward
    (rk_fwfm_backward, then the table scatters).  Inputs after the fixed arguments: the linear
    tables, the embedding tables, field_weight, bias."""

    @staticmethod
    def forward(ctx, model, idx, want_logit, *params):
        F = model.num_fields
        lin_w, emb_w = params[:F], params[F:2 * F]
        field_weight, bias = params[2 * F], params[2 * F + 1]
        B, dev = idx[0].shape[0], idx[0].device
        zeros = [0] * F
        emb = ops.table_seg_array(emb_w, idx, zeros)
        lin = ops.table_seg_array(lin_w, idx, zeros)
        prob = torch.empty(B, device=dev, dtype=torch.float32)
        logit = torch.empty(B, device=dev, dtype=torch.float32) if want_logit else None
        ops.fwfm_forward(emb, lin, model.embed_dim, B, field_weight, bias, logit, prob)
        ctx.model, ctx.idx = model, idx
        ctx.save_for_backward(prob, field_weight, *emb_w, *lin_w)
        if want_logit:
            ctx.mark_non_differentiable(logit)
            return prob, logit
        return prob

    @staticmethod
    def backward(ctx, dprob, *_):
        model, idx = ctx.model, ctx.idx
        F, D = model.num_fields, model.embed_dim
        prob, field_weight, *tabs = ctx.saved_tensors
        emb_w, lin_w = tabs[:F], tabs[F:]
        B, dev = prob.shape[0], prob.device
        f32 = dict(device=dev, dtype=torch.float32)
        d_emb = torch.empty(B, F * D, **f32)
        dz = torch.empty(B, 1, **f32)
        d_r = torch.empty_like(field_weight)
        d_b = torch.empty(1, **f32)
        ops.fwfm_backward(ops.table_seg_array(emb_w, idx, [0] * F), D, B, field_weight, prob,
                          _grad_out(dprob, prob), d_emb, dz, d_r, d_b)
        if model.sparse_grad:  # both table sets in one packing launch
            g = sparse_embedding_grads(list(lin_w) + list(emb_w), [[(i, dz, 0)] for i in idx]
                                       + [[(i, d_emb, f * D)] for f, i in enumerate(idx)])
            g_lin, g_emb = g[:F], g[F:]
        else:
            g_emb = embedding_grads(list(emb_w), idx, 0, d_emb)
            g_lin = embedding_grads(list(lin_w), idx, 0, dz, cols=[0] * F)
        return (None, None, None, *g_lin, *g_emb, d_r, d_b)


def fwfm_train_forward(model, idx, want_logit):
    params = ([m.weight for m in model.linear] + [m.weight for m in model.embedding]
              + [model.field_weight, model.bias])
    return _FwFMTrain.apply(model, idx, want_logit, *params)


# ---------------------------------------------------------------- optimizer

class Adam(torch.optim.Optimizer):
    """torch.optim.Adam with the update as one rk_adam_step launch over all tensors of a group.
    Same constructor, param_groups and state layout (`step`, `exp_avg`, `exp_avg_sq`), so state
    dicts move between this class and torch.optim.Adam.  amsgrad / maximize / differentiable /
    sparse gradients are not implemented and raise."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 maximize=False, foreach=None, capturable=False, differentiable=False, fused=None):
        if amsgrad or maximize or differentiable:
            raise NotImplementedError("rankops.Adam: amsgrad / maximize / differentiable are not implemented")
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused)
        super().__init__(params, defaults)

    def step(self, closure=None):
        """torch.optim's step wrapper (a record_function scope and the step hooks) is taken only when
        a profiler or a hook is there to see it: on the eager loop its cost is of the order of the
        fused update itself."""
        if (torch.autograd.profiler._is_profiler_enabled or _optim_mod._global_optimizer_pre_hooks
                or _optim_mod._global_optimizer_post_hooks or self._optimizer_step_pre_hooks
                or self._optimizer_step_post_hooks):
            return _hooked_step(self, closure)
        return self._step(closure)

    step.hooked = True  # torch.optim.Optimizer._patch_step_function: do not wrap again

    def zero_grad(self, set_to_none: bool = True):
        """Optimizer.zero_grad; with set_to_none (the default, the reference's loop) a plain reset of
        every .grad outside a profiler."""
        if not set_to_none or torch.autograd.profiler._is_profiler_enabled:
            return super().zero_grad(set_to_none)
        for group in self.param_groups:
            for p in group["params"]:
                p.grad = None

    @torch.no_grad()
    def _step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            if not group["capturable"] and self._fast_step(gi, group):
                continue
            if self.__dict__.get("_fast", {}).pop(gi, None) is not None:
                # the general path moves step counts one parameter at a time: give every parameter
                # its own step tensor again (the fast path shares one per group)
                for p in group["params"]:
                    st = self.state.get(p)
                    if st and "step" in st:
                        st["step"] = st["step"].clone()
            beta1, beta2 = group["betas"]
            capturable = group["capturable"]
            by_step = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise NotImplementedError("rankops.Adam: sparse gradients")
                if p.device.type != "cuda" or p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("rankops.Adam: parameters must be contiguous float32 ROCm tensors")
                state = self.state[p]
                if len(state) == 0:
                    # torch's layout: a float32 step tensor, on the device when capturable
                    state["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if capturable \
                        else torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                g = p.grad if p.grad.is_contiguous() and p.grad.dtype == torch.float32 else \
                    p.grad.to(torch.float32).contiguous()
                if capturable:  # incremented on the device by rk_adam_step: graph-capturable
                    if state["step"].device != p.device:
                        state["step"] = state["step"].to(p.device)
                    by_step.setdefault(0, []).append((p, g, state["exp_avg"], state["exp_avg_sq"], state["step"]))
                else:
                    if state["step"].device.type != "cpu":
                        state["step"] = state["step"].cpu()
                    state["step"] += 1
                    by_step.setdefault(int(state["step"].item()), []).append(
                        (p, g, state["exp_avg"], state["exp_avg_sq"]))
            for step, entries in by_step.items():
                dev = entries[0][0].device
                ops.adam_step(entries, float(group["lr"]), beta1, beta2, group["eps"], group["weight_decay"], step,
                              ops._lib.raw_stream(dev))
                # the kernel wrote through raw pointers: bump the version counters as torch's
                # in-place ops would, so weight-derived caches (packed MLP images) are rebuilt
                torch.autograd.graph.increment_version([t for e in entries for t in (e[0], e[2], e[3])])
        return loss

    def _fast_step(self, gi, group) -> bool:
        """The eager step with the marshalled rk_adam_step argument block reused: valid while the
        group's parameters and their states stay the same and every parameter is at the same step
        count (the reference's loop: every parameter gets a gradient every step); new gradient
        storages are patched into the block.  Per step: one increment of the shared CPU step tensor,
        one launch, one version bump.  Anything else (first step, a missing gradient, mixed step
        counts) takes the general path, which rebuilds the block next time."""
        params = group["params"]
        grads = [p.grad for p in params]
        if not params or any(g is None or g.is_sparse for g in grads):  # sparse: the general path raises
            return False
        cache = self.__dict__.setdefault("_fast", {})
        key = tuple(p.data_ptr() for p in params)
        gkey = tuple(g.data_ptr() for g in grads)
        hit = cache.get(gi)
        if hit is not None and hit[0] == key and hit[7] != gkey:
            # new gradient storages (the caching allocator need not hand last step's addresses back
            # after zero_grad(set_to_none=True)): patch the pointers into the block, no rebuild
            if any(g.dtype != torch.float32 or not g.is_contiguous() or g.is_sparse or g.numel() != p.numel()
                   or g.device != p.device for g, p in zip(grads, params)):
                return False
            arr = hit[1]
            for i, g in enumerate(grads):
                arr[i].grad = g.data_ptr()
            hit[7] = gkey
        if hit is None or hit[0] != key:
            states = [self.state.get(p) for p in params]
            if any(not st for st in states) or any(st["step"].device.type != "cpu" for st in states):
                cache.pop(gi, None)
                return False
            if any(g.dtype != torch.float32 or not g.is_contiguous() or g.is_sparse for g in grads) or \
                    any(p.device.type != "cuda" or p.dtype != torch.float32 or not p.is_contiguous() for p in params):
                return False
            counts = {float(st["step"]) for st in states}
            if len(counts) != 1:
                return False
            # one step tensor object for the group (all counts are equal here): a step is then one
            # in-place add instead of a foreach over every parameter's CPU scalar
            shared = states[0]["step"]
            for st in states:
                st["step"] = shared
            entries = [(p, g, st["exp_avg"], st["exp_avg_sq"]) for p, g, st in zip(params, grads, states)]
            arr = (ops._lib.AdamTensor * len(entries))(*[
                ops._lib.AdamTensor(e[0].data_ptr(), e[1].data_ptr(), e[2].data_ptr(), e[3].data_ptr(), e[0].numel(),
                                    None) for e in entries])
            bumped = [t for e in entries for t in (e[0], e[2], e[3])]
            # the block keeps raw gradient pointers only: holding the gradient tensors would keep
            # last step's storages alive across zero_grad(set_to_none=True), so the next backward
            # could never get the same addresses and the key would miss every step
            hit = [key, arr, len(entries), shared, int(counts.pop()), bumped, params[0].device, gkey]
            cache[gi] = hit
            self._fast_builds = getattr(self, "_fast_builds", 0) + 1
        _key, arr, n, step_t, count, bumped, dev, _gkey = hit
        step_t.add_(1.0)
        hit[4] = count = count + 1
        beta1, beta2 = group["betas"]
        ops.check(ops._lib.load().rk_adam_step(arr, n, float(group["lr"]), beta1, beta2, group["eps"],
                                               group["weight_decay"], count,
                                               ops._lib.raw_stream(dev)), "rk_adam_step")
        torch.autograd.graph.increment_version(bumped)
        return True

    def load_state_dict(self, state_dict):
        self.__dict__.pop("_fast", None)  # new state tensors: rebuild the argument blocks
        return super().load_state_dict(state_dict)

    def state_dict(self):
        """Optimizer.state_dict with a step tensor of its own per parameter (the fast path shares
        one per group; another optimizer loading the dict must not see them aliased)."""
        sd = super().state_dict()  # its per-parameter dicts are the live ones: hand out copies
        sd["state"] = {k: ({**st, "step": st["step"].clone()} if "step" in st else dict(st))
                       for k, st in sd["state"].items()}
        return sd


class SparseAdam(torch.optim.Optimizer):
    """torch.optim.SparseAdam (= TF LazyAdamOptimizer's arithmetic, DIEN/dien.py:328) with the update
    of all tables of a group as one rk_sparse_adam_step call: only the rows in a table's sparse
    gradient are read and written, whatever the table's size.  Same constructor arguments and
    state layout (`step`, `exp_avg`, `exp_avg_sq`), so state dicts move between this class and
    torch.optim.SparseAdam.  It takes any sparse COO gradient of a [V, D] float32 table: the
    engine's (model(..., sparse_grad=True)) or nn.Embedding(sparse=True)'s under torch autograd;
    a gradient for which is_coalesced() holds skips the sort.  maximize is not implemented and
    raises; dense gradients raise as torch's do.

    capturable=True keeps the step count on the device, so a whole step can be captured with
    torch.cuda.graph and replayed.  The parameters of a group that are at the same count share
    one float32 counter (one rk_sparse_adam_step call per counter): new parameters and counts
    loaded from a state dict join the group's counter at their count, and a parameter without a
    gradient in a step leaves the shared counter, as torch counts a parameter's steps only when it
    has a gradient (it is then stepped by a call of its own).  state_dict() hands out torch's int
    per parameter and leaves the live counters alone.  Take one eager step before capturing: it
    creates the state and the workspace."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, maximize=False, *, capturable=False):
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not 0.0 < lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 < eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if maximize:
            raise NotImplementedError("rankops.SparseAdam: maximize is not implemented")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, maximize=maximize, capturable=bool(capturable)))
        bad = [[gi, pi] for gi, group in enumerate(self.param_groups) for pi, p in enumerate(group["params"])
               if p.is_sparse or p.is_complex()]
        if bad:
            raise ValueError(f"Sparse or complex params at indices {bad}: SparseAdam requires dense real "
                             "parameter tensors")
        self._workspace = {}  # device -> uint8 tensor, allocated on first use and reused

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("_workspace", {})
        for group in self.param_groups:
            group.setdefault("capturable", False)

    @staticmethod
    def _count(step) -> int:
        return int(step.item()) if isinstance(step, torch.Tensor) else int(step)

    @staticmethod
    def _is_counter(step, p) -> bool:
        return isinstance(step, torch.Tensor) and step.device == p.device and step.dtype == torch.float32

    def _group_counters(self, group):
        """(device, count) -> the device counter the group's parameters already hold at that count
        (reads the counters: only when a parameter has to be given one)."""
        found = {}
        for p in group["params"]:
            st = self.state.get(p)
            if st and self._is_counter(st.get("step"), p):
                found.setdefault((p.device, self._count(st["step"])), st["step"])
        return found

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            capturable = group.get("capturable", False)
            calls = {}      # step count, or id of the device counter -> [counter, entries]
            counters = None  # (device, count) -> device counter, filled when a parameter needs one
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not g.is_sparse:
                    raise RuntimeError("SparseAdam does not support dense gradients, please consider Adam instead")
                if p.device.type != "cuda" or p.dtype != torch.float32 or p.dim() != 2 or not p.is_contiguous():
                    raise RuntimeError("rankops.SparseAdam: parameters must be contiguous 2-D float32 ROCm tensors")
                if g.sparse_dim() != 1 or g.dense_dim() != 1 or g.shape != p.shape or g.device != p.device:
                    raise RuntimeError("rankops.SparseAdam: a gradient must be a sparse COO tensor of its "
                                       "parameter's shape with one sparse dimension (rows)")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                idx, val = g._indices()[0], g._values()
                if val.dtype != torch.float32:
                    val = val.to(torch.float32)
                if val.dim() == 2 and val.shape[1] > 1 and val.stride(1) != 1:
                    val = val.contiguous()
                entry = (p, state["exp_avg"], state["exp_avg_sq"], idx, val, g.is_coalesced())
                if capturable:
                    st = state["step"]
                    if not self._is_counter(st, p):
                        # a new parameter, or a loaded int: join the group's counter at that count
                        if counters is None:
                            counters = self._group_counters(group)
                        key = (p.device, self._count(st))
                        st = counters.get(key)
                        if st is None:
                            st = counters[key] = torch.full((), float(key[1]), dtype=torch.float32, device=p.device)
                        state["step"] = st
                    calls.setdefault(id(st), [st, []])[1].append(entry)
                else:
                    n = state["step"] = self._count(state["step"]) + 1
                    calls.setdefault(n, [None, []])[1].append(entry)
            if capturable:
                # torch counts a parameter's steps only when it has a gradient: one that misses this
                # step leaves the shared counter and keeps its count in a counter of its own
                left = {}
                for p in group["params"]:
                    st = self.state.get(p) if p.grad is None else None
                    if st and id(st.get("step")) in calls:
                        st["step"] = left.setdefault(id(st["step"]), st["step"].clone())
            for key, (counter, entries) in calls.items():
                dev = entries[0][0].device
                self._workspace[dev] = ops.sparse_adam_step(
                    entries, float(group["lr"]), beta1, beta2, group["eps"], 0 if counter is not None else key,
                    ops._lib.raw_stream(dev), device_step=counter, workspace=self._workspace.get(dev))
                # the kernel wrote through raw pointers: bump the version counters as torch's in-place
                # ops would, so weight-derived caches (packed weight images) are rebuilt
                torch.autograd.graph.increment_version([t for e in entries for t in e[:3]])
        return loss

    def load_state_dict(self, state_dict):
        """Optimizer.load_state_dict; a dict written by torch.optim.SparseAdam has no `capturable`
        entry, so every group keeps its own."""
        keep = [group.get("capturable", False) for group in self.param_groups]
        super().load_state_dict(state_dict)
        for group, capturable in zip(self.param_groups, keep):
            group["capturable"] = capturable

    def state_dict(self):
        """Optimizer.state_dict with torch.optim.SparseAdam's int step per parameter.  The returned
        per-parameter dicts are copies: the optimizer's own state (the shared device counters a
        captured step writes to) is left as it is."""
        sd = super().state_dict()
        sd["state"] = {k: ({**st, "step": self._count(st["step"])} if "step" in st else dict(st))
                       for k, st in sd["state"].items()}
        return sd


_hooked_step = torch.optim.Optimizer.profile_hook_step(Adam._step)
