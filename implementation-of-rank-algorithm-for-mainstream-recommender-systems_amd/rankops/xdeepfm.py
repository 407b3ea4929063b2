"""xDeepFM on the rankops engine: DeepFM with the scalar FM term replaced by the Compressed
Interaction Network (Lian et al. 2018, eq. 6-8, "direct" form, no split-half).

The reference's README lists the model; its script is not in the snapshot, so the definition is this
one, in the conventions of the reference's DeepFM (algorithm/DeepFM/deepfm.py):

`XDeepFM(vocab_dir, embedding_dim=8, hidden_units=None, cin_layer_sizes=None,
         cin_activation="identity", dropout_rate=0.1, batch_norm=True, *, vocab_sizes=None,
         trainable=False, sparse_grad=False)`
`forward(category) -> (probability, total_logit, linear_logit, cin_logit, deep_logit)`, each [B, 1].

Modules are created in the order first_order_embeddings, second_order_embeddings, deep_layers,
deep_output_layer, final_layer = Linear(3, 1) — DeepFM's names, shapes and order, so a DeepFM
state_dict loads into them (strict=False) and the same seed gives the same values — then
cin_layers = ModuleList(Conv1d(H_{k-1} m, H_k, 1)) with H_0 = m fields, and
cin_output_layer = Linear(sum H_k, 1).  With x0 = the stacked second-order rows [B, m, D]:

    z[b, h m + i, d] = x^{k-1}[b, h, d] * x0[b, i, d]
    x^k[b, n, d]     = act(sum_j W_k[n, j] z[b, j, d] + bias_k[n])          act: identity | relu
    cin_logit        = cin_output_layer(concat_k sum_d x^k[b, :, d])
    linear_logit     = DeepFM's first-order sum,  deep_logit = DeepFM's deep part on x0.reshape(B, m D)
    total_logit      = final_layer(cat[linear_logit, cin_logit, deep_logit]),  probability = sigmoid(total_logit)

Launches (eval): rk_cin_forward (row gather, first-order sum, every CIN layer on FP32 MFMA with the
feature maps in LDS, pooling, cin_output_layer), then the deep tail (common.tail_launches /
run_tail) whose head epilogue is DeepFM's with fm2 = cin_logit.

Training is opt-in: `XDeepFM(..., trainable=True)` in train mode returns the five outputs attached to
autograd (rankops.train._XDeepFMTrain: rk_cin_forward_train keeps the feature maps, DeepFM's train
tail with batch statistics and Dropout, then rk_cin_backward and rk_cin_wgrad), and under no_grad
runs the same forward keeping nothing; `sparse_grad=True` hands the tables sparse COO gradients
(rankops.SparseAdam) as in DeepFM.  The default (trainable=False) raises NotImplementedError in train
mode, as before.  Neither flag adds, reorders or re-initialises a parameter.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import common, ops, train
from .common import EngineModule, Layer, check_eval, run_tail, table_rows
from .deepfm import WECHAT_FIELDS

CIN_ACTIVATIONS = ("identity", "relu")
# argument slots of the rk_cin_forward launch patched per call (ops.cin_forward_args)
_FM1_SLOT, _CIN_SLOT = 14, 17


class XDeepFM(EngineModule):
    def __init__(self, vocab_dir, embedding_dim=8, hidden_units=None, cin_layer_sizes=None,
                 cin_activation="identity", dropout_rate=0.1, batch_norm=True, *, vocab_sizes=None,
                 trainable=False, sparse_grad=False):
        super().__init__()
        self.trainable = bool(trainable)      # train mode runs the HIP train forward / backward (rankops.train)
        self.sparse_grad = bool(sparse_grad)  # train mode: tables get sparse COO gradients (rankops.SparseAdam)
        if hidden_units is None:
            hidden_units = [512, 256, 128]
        if cin_layer_sizes is None:
            cin_layer_sizes = (128, 128)
        if cin_activation not in CIN_ACTIVATIONS:
            raise ValueError(f"cin_activation must be one of {CIN_ACTIVATIONS}, got {cin_activation!r}")
        if len(cin_layer_sizes) == 0 or any(int(h) <= 0 for h in cin_layer_sizes):
            raise ValueError(f"cin_layer_sizes must be a non-empty list of positive widths, got {cin_layer_sizes!r}")
        if vocab_sizes is not None and any(f not in WECHAT_FIELDS for f in vocab_sizes):
            self.vocab_sizes = {f: int(n) + 1 for f, n in vocab_sizes.items()}
        else:
            self.vocab_sizes = {f: table_rows(vocab_dir, f, vocab_sizes) for f in WECHAT_FIELDS}
        self.num_categories = len(self.vocab_sizes)
        self.embedding_dim = embedding_dim
        self.cin_layer_sizes = tuple(int(h) for h in cin_layer_sizes)
        self.cin_activation = cin_activation
        self.first_order_embeddings = nn.ModuleDict(
            {col: nn.Embedding(n, 1) for col, n in self.vocab_sizes.items()})
        self.second_order_embeddings = nn.ModuleDict(
            {col: nn.Embedding(n, embedding_dim) for col, n in self.vocab_sizes.items()})
        self.deep_layers = nn.ModuleList()
        width = self.num_categories * embedding_dim
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
        self.final_layer = nn.Linear(3, 1)
        self.cin_layers = nn.ModuleList()
        hprev = self.num_categories
        for h in self.cin_layer_sizes:
            self.cin_layers.append(nn.Conv1d(hprev * self.num_categories, h, 1))
            hprev = h
        self.cin_output_layer = nn.Linear(sum(self.cin_layer_sizes), 1)
        self._dropout = train.DropoutStreams()

    def _indices(self, category):
        names = list(self.second_order_embeddings)
        if not isinstance(category, dict):
            raise TypeError(f"XDeepFM.forward: category must be a dict of index tensors, got {type(category).__name__}")
        missing = [c for c in names if c not in category]
        if missing:
            raise KeyError(f"XDeepFM.forward: category features missing: {missing}")
        idx = [ops.as_index(category[n], f"category[{n!r}]") for n in names]
        if any(t.dim() != 1 or t.shape[0] != idx[0].shape[0] for t in idx):
            raise ValueError("XDeepFM.forward: every category feature must be a 1-D tensor of one length")
        return names, idx

    def _build(self, names, idx):
        """The forward's launches over these index tensors as a common.Bound: rk_cin_forward, then the
        fused deep tail (ep None, and no tail launch, when the deep layers are outside it: _run).  The
        outputs are patched in per call."""
        D, m = self.embedding_dim, self.num_categories
        B, dev = idx[0].shape[0], idx[0].device
        second = [ops.table_segment(self.second_order_embeddings[n].weight, i, f * D)
                  for f, (n, i) in enumerate(zip(names, idx))]
        first = [ops.table_segment(self.first_order_embeddings[n].weight, i, f)
                 for f, (n, i) in enumerate(zip(names, idx))]
        images = [common.CIN_PACKED(c.weight) for c in self.cin_layers]
        biases = [c.bias for c in self.cin_layers]
        deep_in = torch.empty(B, m * D, device=dev, dtype=torch.float32)
        args, keep = ops.cin_forward_args(second, first, D, B, images, biases, self.cin_layer_sizes,
                                          self.cin_activation, self.cin_output_layer.weight,
                                          self.cin_output_layer.bias, deep_in, None, None, None, dev)
        head_kwargs = dict(final_w=self.final_layer.weight, final_b=self.final_layer.bias)
        tail = common.tail_launches(deep_in, self._tail, self.deep_output_layer, head_kwargs)
        tl, ep, tkeep = tail if tail is not None else ([], None, None)
        # keep-alive: the deep input (_run reads it), and what the argument blocks point into (not the
        # caller's index tensors: the cache key's address / shape / stride check makes those pointers
        # valid on a hit)
        return common.bound([("rk_cin_forward", args)] + tl, B, dict(deep_in=deep_in, blocks=(keep, images, tkeep)),
                            self._patch, ep)

    @staticmethod
    def _patch(ep, args, out):
        prob, total, linear, cin, deep = out
        args[_FM1_SLOT], args[_CIN_SLOT] = linear.data_ptr(), cin.data_ptr()
        if ep is not None:
            ep.fm1, ep.fm2, ep.head_aux = linear.data_ptr(), cin.data_ptr(), deep.data_ptr()
            ep.head_logit, ep.head_prob = total.data_ptr(), prob.data_ptr()

    def _run(self, bound, out, stream):
        bound.patch(out)
        common.run_launches(bound.launches, stream)
        if bound.ep is None:  # deep layers outside the fused tail: rk_linear per layer
            prob, total, linear, cin, deep = out
            head_kwargs = dict(fm1=linear, fm2=cin, final_w=self.final_layer.weight, final_b=self.final_layer.bias,
                               head_aux=deep)
            run_tail(bound.keep["deep_in"], self._tail, self.deep_output_layer, head_kwargs, total, prob)

    @staticmethod
    def _outputs(B, dev):
        return common.empty_rows(dev, 5, (B, 1))

    def prepare(self, category):
        """An eval forward bound to these input tensors (as DeepFM.prepare): returns `run()` that
        recomputes the whole forward from the current contents of the inputs with the cached launches
        (rk_cin_forward, then the deep tail) and returns the same (probability, total_logit,
        linear_logit, cin_logit, deep_logit) tensors each time.  Binds the current weights and their
        packed images (the CIN layers' and the deep layers'): prepare again after changing them."""
        if self.training:
            raise RuntimeError("XDeepFM.prepare: eval mode only (call .eval() first)")
        names = list(self.second_order_embeddings)
        idx = [ops.bound_index(category[n], f"category[{n!r}]") for n in names]
        if any(t.dim() != 1 or t.shape[0] != idx[0].shape[0] for t in idx):
            raise ValueError("XDeepFM.prepare: every category feature must be a 1-D tensor of one length")
        if idx[0].shape[0] == 0:
            raise ValueError("XDeepFM.prepare: empty batch")
        bound = self._build(names, idx)
        if bound.ep is None:
            raise RuntimeError("XDeepFM.prepare: deep layers outside the fused tail (common.fused_mlp_fits)")
        common.pin_tail(self._tail)  # the images the plan binds are never rewritten in place under it
        for c in self.cin_layers:
            common.CIN_PACKED.pin(c.weight)
        return common.prepared(self, bound, idx[0].device, category)

    def forward(self, category):
        if not self.trainable:
            check_eval(self)  # train mode is opt-in (trainable=True)
        names, idx = self._indices(category)
        B, dev = idx[0].shape[0], idx[0].device
        if B == 0:
            return common.empty_rows(dev, 5)
        if self.training:  # BatchNorm batch statistics, Dropout, HIP backward (rankops.train)
            grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
            return train.xdeepfm_train_forward(self, names, idx, grad)
        stream = ops._lib.raw_stream(dev)
        if all(t is category[n] for t, n in zip(idx, names)):  # no converted copies: addresses are the caller's
            bound = common.EagerCalls.lookup(self, idx, stream, lambda: self._build(names, idx))
        else:
            bound = self._build(names, idx)
        out = self._outputs(B, dev)
        self._run(bound, out, stream)
        return out
