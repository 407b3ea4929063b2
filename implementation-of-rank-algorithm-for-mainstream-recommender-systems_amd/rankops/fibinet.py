"""FiBiNET on the rankops engine (Huang et al., RecSys 2019): SENET field attention over the
second-order rows, a bilinear interaction of the plain and of the re-weighted rows, and DeepFM's deep
part over the two interaction vectors.

The reference's README lists the model; its script is not in the snapshot, so the definition is this
one, in the conventions of the reference's DeepFM (algorithm/DeepFM/deepfm.py) and of rankops.XDeepFM:

`FiBiNET(vocab_dir, embedding_dim=8, hidden_units=None, reduction_ratio=3, bilinear_type="interaction",
         dropout_rate=0.1, batch_norm=True, *, vocab_sizes=None)`
`forward(category) -> (probability, total_logit, linear_logit, deep_logit)`, each [B, 1].

Modules are created in the order first_order_embeddings, second_order_embeddings (DeepFM's names,
shapes and order: the same seed gives DeepFM's tables and a DeepFM state_dict loads them with
strict=False), senet = Sequential(Linear(m, r, bias=False), ReLU, Linear(r, m, bias=False), ReLU) with
r = max(1, m // reduction_ratio), bilinear_embedding and bilinear_senet = ModuleList(Linear(D, D,
bias=False)) of 1 ("all"), m - 1 ("each") or m (m - 1) / 2 ("interaction") matrices, deep_layers (Linear,
BatchNorm1d, ReLU, Dropout per hidden unit, the first m (m - 1) D wide), deep_output_layer, and
final_layer = Linear(2, 1).  With e[b, i, :] the second-order row of field i and the pairs (i, j),
i < j, in lexicographic order:

    z[b, i]    = mean_d e[b, i, d]
    a[b, :]    = relu(W2 relu(W1 z[b, :]))                   W1 = senet[0].weight, W2 = senet[2].weight
    v[b, i, :] = a[b, i] e[b, i, :]
    p[b, p, :] = (We e[b, i, :]) * e[b, j, :]                We = bilinear_embedding[0 | i | p] by type
    q[b, p, :] = (Wv v[b, i, :]) * v[b, j, :]                Wv = bilinear_senet, same indexing
    c[b, :]    = cat(p[b].flatten(), q[b].flatten())
    linear_logit = DeepFM's first-order sum,  deep_logit = deep_output_layer(deep_layers(c))
    total_logit  = final_layer(cat[linear_logit, deep_logit]),  probability = sigmoid(total_logit)

Launches (eval): inside common.fibinet_fits, up to one 16-sample workgroup per CU, the whole forward is
one rk_fibinet_forward launch (row gather, first-order sum, SENET, both bilinear layers into the MLP's
LDS input row, deep layers, head); outside the envelope, at larger batches (where it is faster) or with
`two_launch = True` on the module (False: the one launch at any batch), rk_fibinet_interaction writes c
and the deep tail follows (common.tail_launches / run_tail; its DeepFM head epilogue with the weight image
[w0, 0, w1] is final_layer).  Eval only: train mode raises NotImplementedError.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import common, ops
from .common import EngineModule, Layer, check_eval, run_tail, table_rows
from .deepfm import WECHAT_FIELDS

BILINEAR_TYPES = tuple(ops.FIBINET_TYPES)


class FiBiNET(EngineModule):
    def __init__(self, vocab_dir, embedding_dim=8, hidden_units=None, reduction_ratio=3,
                 bilinear_type="interaction", dropout_rate=0.1, batch_norm=True, *, vocab_sizes=None):
        super().__init__()
        if hidden_units is None:
            hidden_units = [512, 256, 128]
        if bilinear_type not in BILINEAR_TYPES:
            raise ValueError(f"bilinear_type must be one of {BILINEAR_TYPES}, got {bilinear_type!r}")
        if int(reduction_ratio) < 1:
            raise ValueError(f"reduction_ratio must be at least 1, got {reduction_ratio!r}")
        if vocab_sizes is not None and any(f not in WECHAT_FIELDS for f in vocab_sizes):
            self.vocab_sizes = {f: int(n) + 1 for f, n in vocab_sizes.items()}
        else:
            self.vocab_sizes = {f: table_rows(vocab_dir, f, vocab_sizes) for f in WECHAT_FIELDS}
        m = self.num_categories = len(self.vocab_sizes)
        self.embedding_dim = embedding_dim
        self.bilinear_type = bilinear_type
        self.reduced = max(1, m // int(reduction_ratio))
        # None: the faster path at each batch size (fused()); True: always rk_fibinet_interaction + the deep tail;
        # False: the one launch wherever the kernel takes the shape
        self.two_launch = None
        self.first_order_embeddings = nn.ModuleDict(
            {col: nn.Embedding(n, 1) for col, n in self.vocab_sizes.items()})
        self.second_order_embeddings = nn.ModuleDict(
            {col: nn.Embedding(n, embedding_dim) for col, n in self.vocab_sizes.items()})
        self.senet = nn.Sequential(nn.Linear(m, self.reduced, bias=False), nn.ReLU(),
                                   nn.Linear(self.reduced, m, bias=False), nn.ReLU())
        nmat = ops.fibinet_matrices(m, bilinear_type)
        self.bilinear_embedding = nn.ModuleList(
            [nn.Linear(embedding_dim, embedding_dim, bias=False) for _ in range(nmat)])
        self.bilinear_senet = nn.ModuleList(
            [nn.Linear(embedding_dim, embedding_dim, bias=False) for _ in range(nmat)])
        self.deep_layers = nn.ModuleList()
        width = self.interaction_width = m * (m - 1) * embedding_dim
        self._tail = []
        for unit in hidden_units:
            lin = nn.Linear(width, unit)
            self.deep_layers.append(lin)
            bn = None
            if batch_norm:
                bn = nn.BatchNorm1d(unit)
                self.deep_layers.append(bn)
            self.deep_layers.append(nn.ReLU())
            if dropout_rate > 0:
                self.deep_layers.append(nn.Dropout(dropout_rate))
            self._tail.append(Layer(lin, pre_bn=bn, act="relu"))
            width = unit
        self.deep_output_layer = nn.Linear(width, 1)
        self.final_layer = nn.Linear(2, 1)
        self._stack_e, self._stack_v, self._final3 = common.Packed(), common.Packed(), common.Packed()

    def fused(self, batch=None, device=None) -> bool:
        """Whether the eval forward (of this batch, when given) is the single rk_fibinet_forward launch:
        inside the kernel's envelope, and, unless two_launch is False, a batch that gives no CU a second
        16-sample workgroup (past that the two launches are faster: DESIGN.md §4g)."""
        if self.two_launch or not (common.FUSED_MLP and common.fibinet_fits(
                self.num_categories, self.embedding_dim, self.reduced, self.bilinear_type,
                [l.linear.out_features for l in self._tail])):
            return False
        per_cu = common.FUSED_FIBINET_WG_PER_CU
        if self.two_launch is False or batch is None or per_cu is None:
            return True
        return (batch + 15) // 16 <= per_cu * common._num_cus(device)

    def _indices(self, category):
        names = list(self.second_order_embeddings)
        if not isinstance(category, dict):
            raise TypeError(f"FiBiNET.forward: category must be a dict of index tensors, got {type(category).__name__}")
        missing = [c for c in names if c not in category]
        if missing:
            raise KeyError(f"FiBiNET.forward: category features missing: {missing}")
        idx = [ops.as_index(category[n], f"category[{n!r}]") for n in names]
        if any(t.dim() != 1 or t.shape[0] != idx[0].shape[0] for t in idx):
            raise ValueError("FiBiNET.forward: every category feature must be a 1-D tensor of one length")
        return names, idx

    def _build(self, names, idx):
        """The forward's launches over these index tensors as a common.Bound: rk_fibinet_forward alone, or
        rk_fibinet_interaction and the fused deep tail (ep None, and no tail launch, when the deep layers
        are outside it: _run).  The outputs are patched in per call."""
        D, m = self.embedding_dim, self.num_categories
        B, dev = idx[0].shape[0], idx[0].device
        second = [ops.table_segment(self.second_order_embeddings[n].weight, i, f * D)
                  for f, (n, i) in enumerate(zip(names, idx))]
        first = [ops.table_segment(self.first_order_embeddings[n].weight, i, f)
                 for f, (n, i) in enumerate(zip(names, idx))]
        w1, w2 = self.senet[0].weight.detach(), self.senet[2].weight.detach()
        be = self._stack_e(*[l.weight for l in self.bilinear_embedding])  # [nmat D, D] = the stacked [nmat, D, D]
        bv = self._stack_v(*[l.weight for l in self.bilinear_senet])
        if self.fused(B, dev):
            mls, images = common.tail_layers(self._tail)
            args, keep = ops.fibinet_forward_args(second, first, D, B, w1, w2, be, bv, self.bilinear_type, mls,
                                                  self.deep_output_layer.weight, self.deep_output_layer.bias,
                                                  self.final_layer.weight, self.final_layer.bias, dev)
            return common.bound([("rk_fibinet_forward", args)], B, dict(blocks=(keep, images, mls, be, bv, w1, w2)),
                                self._patch_fused)
        c = torch.empty(B, self.interaction_width, device=dev, dtype=torch.float32)
        args, keep = ops.fibinet_interaction_args(second, first, D, B, w1, w2, be, bv, self.bilinear_type, c, None,
                                                  None, dev)
        tail = common.tail_launches(c, self._tail, self.deep_output_layer, self._head_kwargs())
        tl, ep, tkeep = tail if tail is not None else ([], None, None)
        return common.bound([("rk_fibinet_interaction", args)] + tl, B,
                            dict(c=c, blocks=(keep, tkeep, be, bv, w1, w2)), self._patch_split, ep)

    def _head_kwargs(self):
        """final_layer = Linear(2, 1) as the DeepFM combine of the tail's head epilogue: the weight image
        [w0, 0, w1] over (fm1, fm2, deep) with fm1 = fm2 = linear_logit (0 * linear adds an exact zero)."""
        w = self.final_layer.weight
        zero = common.const(w.device, 0.0).view(1, 1)
        return dict(final_w=self._final3(w[:, :1], zero, w[:, 1:]), final_b=self.final_layer.bias)

    @staticmethod
    def _patch_fused(ep, args, out):
        for slot, o in zip(ops.FIBINET_OUT_SLOTS, out):  # (probability, total_logit, linear_logit, deep_logit)
            args[slot] = o.data_ptr()

    @staticmethod
    def _patch_split(ep, args, out):
        prob, total, linear, deep = out
        args[ops.FIBINET_LINEAR_SLOT] = linear.data_ptr()
        if ep is not None:
            ep.fm1, ep.fm2, ep.head_aux = linear.data_ptr(), linear.data_ptr(), deep.data_ptr()
            ep.head_logit, ep.head_prob = total.data_ptr(), prob.data_ptr()

    def _run(self, bound, out, stream):
        bound.patch(out)
        common.run_launches(bound.launches, stream)
        if bound.ep is None and "c" in bound.keep:  # deep layers outside the fused tail: rk_linear per layer
            prob, total, linear, deep = out
            run_tail(bound.keep["c"], self._tail, self.deep_output_layer,
                     dict(self._head_kwargs(), fm1=linear, fm2=linear, head_aux=deep), total, prob)

    @staticmethod
    def _outputs(B, dev):
        return common.empty_rows(dev, 4, (B, 1))

    def prepare(self, category):
        """An eval forward bound to these input tensors (as XDeepFM.prepare): returns `run()` that
        recomputes the whole forward from the current contents of the inputs with the cached launches
        (rk_fibinet_forward, or rk_fibinet_interaction and the deep tail) and returns the same
        (probability, total_logit, linear_logit, deep_logit) tensors each time.  Binds the current
        weights, the stacked bilinear matrices and the packed images of the deep layers: prepare again
        after changing them."""
        if self.training:
            raise RuntimeError("FiBiNET.prepare: eval mode only (call .eval() first)")
        names = list(self.second_order_embeddings)
        idx = [ops.bound_index(category[n], f"category[{n!r}]") for n in names]
        if any(t.dim() != 1 or t.shape[0] != idx[0].shape[0] for t in idx):
            raise ValueError("FiBiNET.prepare: every category feature must be a 1-D tensor of one length")
        if idx[0].shape[0] == 0:
            raise ValueError("FiBiNET.prepare: empty batch")
        bound = self._build(names, idx)
        if bound.ep is None and "c" in bound.keep:
            raise RuntimeError("FiBiNET.prepare: deep layers outside the fused tail (common.fused_mlp_fits)")
        common.pin_tail(self._tail)  # the images the plan binds are never rewritten in place under it
        return common.prepared(self, bound, idx[0].device, category)

    def forward(self, category):
        check_eval(self)
        names, idx = self._indices(category)
        B, dev = idx[0].shape[0], idx[0].device
        if B == 0:
            return common.empty_rows(dev, 4)
        stream = ops._lib.raw_stream(dev)
        if all(t is category[n] for t, n in zip(idx, names)):  # no converted copies: addresses are the caller's
            bound = common.EagerCalls.lookup(self, idx, stream, lambda: self._build(names, idx),
                                             extra=(self.two_launch,))
        else:
            bound = self._build(names, idx)
        out = self._outputs(B, dev)
        self._run(bound, out, stream)
        return out
