"""Deep Crossing on the rankops engine — drop-in for algorithm/DeepCrossing/deepcrossing.py.

`DeepCrossingModel(vocab_dir, residual_internal_dim=128, residual_network_num=1)` keeps the
reference constructor, state_dict keys (`embeddings.*`, `output_layer.*`; the residual units
have none, deepcrossing.py:106-137) and `forward(dense, category) -> (probability, logit)`
(deepcrossing.py:146-163).

Launches: rk_concat_gather -> x0 [B, 50]; per residual unit two rk_linear calls
(Linear+ReLU, then Linear + residual + ReLU), the last one also evaluating output_layer and
the sigmoid in its epilogue.  The residual units' Linear layers are drawn per call from the
CPU generator like the reference (deepcrossing.py:37-39) or frozen.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops, train
from . import common
from .common import InteractionWeights, check_eval, const, draw_residual_units, fused_mlp_fits, load_vocabulary, residual_spec, \
    table_rows


def residual_unit(input_tensor, internal_dim, index, weights=None):
    """Reference residual_unit (deepcrossing.py:25-42): ReLU(x + Linear2(ReLU(Linear1(x))))."""
    x = ops.as_f32(input_tensor, "input_tensor")
    B, d = x.shape
    if weights is None:
        weights = [t.to(x.device) for t in draw_residual_units(d, internal_dim, 1)[0]]
    w1, b1, w2, b2 = weights
    h = torch.empty(B, internal_dim, device=x.device, dtype=torch.float32)
    ops.linear(x, w1, h, epilogue=ops.make_epilogue(bias=b1, act="relu"))
    out = torch.empty(B, d, device=x.device, dtype=torch.float32)
    ops.linear(h, w2, out, epilogue=ops.make_epilogue(bias=b2, residual=x, ld_residual=x.stride(0), act="relu"))
    return out


class DeepCrossingModel(common.EngineModule):
    def __init__(self, vocab_dir, residual_internal_dim=128, residual_network_num=1, *, vocab_sizes=None,
                 interaction_weights="per_call", sparse_grad=False):
        super().__init__()
        self.sparse_grad = bool(sparse_grad)  # train mode: tables get sparse COO gradients (rankops.SparseAdam)
        fields = ("userid", "feedid", "device", "authorid", "bgm_song_id", "bgm_singer_id", "manual_tag_list")
        self.vocab_sizes = {f: table_rows(vocab_dir, f, vocab_sizes) for f in fields}
        self.num_dense_features = 16
        self.embeddings = nn.ModuleDict({
            "userid": nn.Embedding(self.vocab_sizes["userid"], 16),
            "device": nn.Embedding(self.vocab_sizes["device"], 2),
            "authorid": nn.Embedding(self.vocab_sizes["authorid"], 4),
            "bgm_song_id": nn.Embedding(self.vocab_sizes["bgm_song_id"], 4),
            "bgm_singer_id": nn.Embedding(self.vocab_sizes["bgm_singer_id"], 4),
            "manual_tag_list": nn.Embedding(self.vocab_sizes["manual_tag_list"], 4),
        })
        self.input_dim = self.num_dense_features + 16 + 2 + 4 + 4 + 4 + 4
        self.residual_internal_dim = residual_internal_dim
        self.residual_network_num = residual_network_num
        self.output_layer = nn.Linear(self.input_dim, 1)
        self.residual_weights = InteractionWeights(
            interaction_weights,
            lambda: residual_spec(self.input_dim, self.residual_internal_dim, self.residual_network_num))

    def _load_vocabulary(self, vocab_dir, filename):
        return load_vocabulary(vocab_dir, filename)

    def _fits(self, units) -> bool:
        """Whether the residual units run as the fused MLP (rk_mlp_forward / rk_mlp_forward_gather)."""
        widths = [w for _ in units for w in (self.residual_internal_dim, self.input_dim)]
        return bool(units and common.FUSED_MLP and fused_mlp_fits(self.input_dim, widths))

    @staticmethod
    def _mlp_layers(units):
        """rk_mlp_layer records of the residual units, and their packed images (common.PACKED)."""
        layers, packed = [], []
        for w1, b1, w2, b2 in units:
            for w, b, residual in ((w1, b1, 0), (w2, b2, 1)):
                packed.append(common.PACKED(w))
                layers.append(ops.make_mlp_layer(w, packed[-1], bias=b, act="relu", residual=residual))
        return layers, packed

    def _segments(self, dense, idxs):
        segs = [ops.dense_segment(dense, self.num_dense_features, 0)]
        col = self.num_dense_features
        for emb, idx in zip(self.embeddings.values(), idxs):
            segs.append(ops.table_segment(emb.weight, idx, col))
            col += emb.embedding_dim
        return segs

    def _build(self, dense, idxs, units):
        """The one-launch eval forward (rk_mlp_forward_gather: row gather + every residual unit +
        output_layer + sigmoid) bound to `dense`, the index tensors `idxs` (table order) and the
        residual weights `units` as a common.Bound; None outside the launch's envelope.  The outputs
        are patched in per call (_patch)."""
        if not (self._fits(units) and len(idxs) < 16 and self.input_dim <= 256):
            return None
        B, dev = dense.shape[0], dense.device
        ep = ops.make_epilogue(head_w=self.output_layer.weight, head_b=self.output_layer.bias)
        layers, packed = self._mlp_layers(units)
        args = ops.mlp_forward_gather_args(self._segments(dense, idxs), self.input_dim, B, layers, ep, dev)
        return common.bound([("rk_mlp_forward_gather", args)], B, (packed, units, idxs), self._patch, ep)

    @staticmethod
    def _patch(ep, _args, out):
        prob, logit = out
        ep.head_logit, ep.head_prob = logit.data_ptr(), prob.data_ptr()

    @staticmethod
    def _outputs(B, dev):
        return common.empty_rows(dev, 2, (B, 1))

    def prepare(self, dense, category):
        """An eval forward bound to these input tensors (as DCNModel.prepare): returns `run()` that
        recomputes the forward from the current contents of the inputs with one
        rk_mlp_forward_gather launch (row gather + every residual unit + output_layer + sigmoid) and
        returns the same (prob, logit) tensors each time.  Binds the current weights: the residual
        units' and the output layer's packed images are pinned, so a later weight update is not seen
        by run() (prepare again after an update).  Frozen residual weights only (per-call mode redraws
        them every forward).  Index tensors must be int64 (bound by address, never copied)."""
        if self.training:
            raise RuntimeError("DeepCrossingModel.prepare: eval mode only (call .eval() first)")
        if self.residual_weights.mode != "frozen":
            raise RuntimeError("DeepCrossingModel.prepare: per-call residual weights are redrawn every forward; "
                               "use interaction_weights='frozen'")
        dense = ops.as_f32(dense, "dense")
        idxs = [ops.bound_index(category[name], f"category[{name!r}]") for name in self.embeddings]
        units = self.residual_weights.get(dense.device)
        bound = self._build(dense, idxs, units)
        if bound is None:
            raise RuntimeError("DeepCrossingModel.prepare: configuration outside rk_mlp_forward_gather's envelope")
        for w1, _, w2, _ in units:  # the images the launch binds are never rewritten in place under it
            common.PACKED.pin(w1)
            common.PACKED.pin(w2)
        return common.prepared(self, bound, dense.device, (dense, category))

    def forward(self, dense, category):
        # no BatchNorm / Dropout: train mode computes the eval forward; with autograd recording it
        # runs under rankops.train._DeepCrossingTrain (HIP backward)
        dense = ops.as_f32(dense, "dense")
        B = dense.shape[0]
        dev = dense.device
        recording = self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if B == 0 and not recording:
            self.residual_weights.get(dev)  # per-call mode draws every forward (deepcrossing.py:25-42)
            return common.empty_rows(dev, 2)
        idxs = []
        for name in self.embeddings:
            if name not in category:
                raise KeyError(f"DeepCrossingModel.forward: category feature {name!r} missing")
            idxs.append(ops.as_index(category[name], f"category[{name!r}]"))
        units = self.residual_weights.get(dev)
        if recording:
            return train.deepcrossing_train_forward(self, dense, idxs, units)
        out = prob, logit = self._outputs(B, dev)
        bound = self._build(dense, idxs, units) if common.FUSED_GATHER_MLP else None
        if bound is not None:
            bound.patch(out)
            common.run_launches(bound.launches, ops._lib.raw_stream(dev))
            return out
        head = dict(head_w=self.output_layer.weight, head_b=self.output_layer.bias, head_logit=logit,
                    head_prob=prob)
        I = self.residual_internal_dim
        x = torch.empty(B, self.input_dim, device=dev, dtype=torch.float32)
        ops.concat_gather(self._segments(dense, idxs), B, x)
        if self._fits(units):
            # all residual units + output_layer + sigmoid in one launch
            ops.mlp_forward(x, self._mlp_layers(units)[0], ops.make_epilogue(**head))
            return out
        for i, (w1, b1, w2, b2) in enumerate(units):
            last = i == len(units) - 1
            h = torch.empty(B, I, device=dev, dtype=torch.float32)
            ops.linear(x, w1, h, epilogue=ops.make_epilogue(bias=b1, act="relu"))
            res = dict(bias=b2, residual=x, ld_residual=x.stride(0), act="relu")
            if last:
                ops.linear(h, w2, None, epilogue=ops.make_epilogue(**res, **head))
            else:
                y = torch.empty(B, self.input_dim, device=dev, dtype=torch.float32)
                ops.linear(h, w2, y, epilogue=ops.make_epilogue(**res))
                x = y
        if not units:
            ep = ops.make_epilogue(bias=self.output_layer.bias, head_w=const(dev, 1.0), head_b=const(dev, 0.0),
                                   head_logit=logit, head_prob=prob)
            ops.linear(x, self.output_layer.weight, None, epilogue=ep)
        return out
