"""MMoE (Multi-gate Mixture-of-Experts, Ma et al., KDD 2018) on the rankops engine: the base of the
reference README's multi-task list (ESMM, MMOE, PLE), one probability per task and row.

The reference's README lists the model; its script is not in the snapshot, so the definition is this
one, in the conventions of the reference's DCN (algorithm/DCN/dcn.py):

`MMoE(vocab_dir, num_experts=4, expert_hidden_units=(256, 128), tower_hidden_units=(64,),
      task_names=("read_comment", "like", "click_avatar"), dropout_rate=0.1, *, vocab_sizes=None,
      trainable=False, sparse_grad=False)`
`forward(dense [B, 16], category {6 x [B]}) -> (probabilities [B, K], logits [B, K])`, column k = task_names[k].

Modules are created in this order (it fixes the seeded values and the state_dict keys):
embeddings (DCNModel's ModuleDict exactly: a DCN checkpoint's `embeddings.*` load, the same seed gives
the same tables), experts = ModuleList of E Sequential(Linear, ReLU, Dropout(p) per hidden unit; no
Dropout when p == 0), gates = ModuleList of K Linear(input_dim, E), towers = ModuleList of K Sequential
built the same way (empty: the identity), tower_outputs = ModuleList of K Linear(last_width, 1).
In eval mode (Dropout the identity), with x = cat[dense, embeddings]:

    f_e = experts[e](x),   g_k = softmax_e(gates[k](x)),   m_k = sum_e g_k[e] f_e   (e ascending)
    logit_k = tower_outputs[k](towers[k](m_k)),   prob_k = sigmoid(logit_k)

One launch, rk_mmoe_forward (csrc/mmoe.hip): the row gather, the K gates as one GEMM and their
softmax, the experts with the mix behind each one's last layer, the towers and the heads; the
[B, E, H] expert outputs, the gates and the mixtures never reach HBM.  CPU tensors raise the engine's
"ROCm GPU" error; a configuration outside the kernel's envelope (common.mmoe_fits) is an error, not a
fallback.

Training is opt-in: `MMoE(..., trainable=True)` in train mode returns (probabilities, logits) attached to
autograd (rankops.train._MMoETrain): rk_mmoe_forward_train, the same kernel with Dropout live behind
every ReLU and the activations kept, then the backward of the heads, towers, mix, gates and experts in a
number of launches that does not depend on E or K (ops.mmoe_backward), and the embedding gradients;
under no_grad it runs the same forward and keeps nothing; `sparse_grad=True` hands the tables sparse
COO gradients (rankops.SparseAdam).  The default (trainable=False) raises NotImplementedError in train
mode, as before.  Neither flag adds, reorders or re-initialises a parameter.  Dropout masks are the
engine's counter hash: with De = len(expert_hidden_units), Dt = len(tower_hidden_units) and (seed, slot)
of the forward (model._dropout), expert e layer l drew `ops.dropout_mask(seed + e * De + l, slot, B, n, p)`
and tower k layer l `ops.dropout_mask(seed + E * De + k * Dt + l, slot, B, n, p)` (element b * n + j).

`rankops.mmoe(x, experts, gates, towers=None)` is the same kernel on plain tensors (ops.mmoe),
differentiable when an input requires grad; this module is callable so that `rankops.mmoe` is both the
module and that function.
"""
from __future__ import annotations

import sys
import types

import torch
import torch.nn as nn

from . import common, ops, train
from .common import EngineModule, check_eval, table_rows

DEFAULT_TASKS = ("read_comment", "like", "click_avatar")


def _stack(width, units, dropout_rate):
    layers = []
    for h in units:
        layers += [nn.Linear(width, h), nn.ReLU()]
        if dropout_rate > 0:
            layers.append(nn.Dropout(dropout_rate))
        width = h
    return nn.Sequential(*layers), width


class MMoE(EngineModule):
    def __init__(self, vocab_dir, num_experts=4, expert_hidden_units=(256, 128), tower_hidden_units=(64,),
                 task_names=DEFAULT_TASKS, dropout_rate=0.1, *, vocab_sizes=None, trainable=False, sparse_grad=False):
        super().__init__()
        self.trainable = bool(trainable)      # train mode runs the HIP train forward / backward (rankops.train)
        self.sparse_grad = bool(sparse_grad)  # train mode: tables get sparse COO gradients (rankops.SparseAdam)
        self.dropout_rate = float(dropout_rate)
        expert_hidden_units = tuple(int(h) for h in expert_hidden_units)
        tower_hidden_units = tuple(int(h) for h in tower_hidden_units)
        task_names = tuple(task_names)
        if int(num_experts) <= 0:
            raise ValueError(f"num_experts must be positive, got {num_experts!r}")
        if len(expert_hidden_units) == 0 or any(h <= 0 for h in expert_hidden_units + tower_hidden_units):
            raise ValueError(f"expert_hidden_units must be a non-empty list of positive widths and tower_hidden_units "
                             f"a list of positive widths, got {expert_hidden_units!r}, {tower_hidden_units!r}")
        if len(task_names) == 0 or len(set(task_names)) != len(task_names):
            raise ValueError(f"task_names must be a non-empty list of distinct names, got {task_names!r}")
        if not 0 <= dropout_rate < 1:
            raise ValueError(f"dropout_rate must lie in [0, 1), got {dropout_rate!r}")
        fields = ("userid", "feedid", "device", "authorid", "bgm_song_id", "bgm_singer_id", "manual_tag_list")
        self.vocab_sizes = {f: table_rows(vocab_dir, f, vocab_sizes) for f in fields}
        self.num_dense_features = 16
        self.num_experts = int(num_experts)
        self.task_names = task_names
        self.expert_hidden_units = expert_hidden_units
        self.tower_hidden_units = tower_hidden_units
        self.embeddings = nn.ModuleDict({
            "userid": nn.Embedding(self.vocab_sizes["userid"], 16),
            "device": nn.Embedding(self.vocab_sizes["device"], 2),
            "authorid": nn.Embedding(self.vocab_sizes["authorid"], 4),
            "bgm_song_id": nn.Embedding(self.vocab_sizes["bgm_song_id"], 4),
            "bgm_singer_id": nn.Embedding(self.vocab_sizes["bgm_singer_id"], 4),
            "manual_tag_list": nn.Embedding(self.vocab_sizes["manual_tag_list"], 4),
        })
        self.input_dim = self.num_dense_features + 16 + 2 + 4 + 4 + 4 + 4
        K = len(task_names)
        self.experts = nn.ModuleList()
        for _ in range(self.num_experts):
            seq, width = _stack(self.input_dim, expert_hidden_units, dropout_rate)
            self.experts.append(seq)
        self.gates = nn.ModuleList(nn.Linear(self.input_dim, self.num_experts) for _ in range(K))
        self.towers = nn.ModuleList()
        last = width
        for _ in range(K):
            seq, last = _stack(width, tower_hidden_units, dropout_rate)
            self.towers.append(seq)
        self.tower_outputs = nn.ModuleList(nn.Linear(last, 1) for _ in range(K))
        self._gate_w, self._gate_b = common.Packed(), common.Packed()  # the K gates stacked to [K E, width]

    def fits(self) -> bool:
        return common.mmoe_fits(self.input_dim, 1 + len(self.embeddings), self.num_experts, len(self.task_names),
                                self.expert_hidden_units, self.tower_hidden_units)

    def _indices(self, category):
        names = list(self.embeddings)
        if not isinstance(category, dict):
            raise TypeError(f"MMoE.forward: category must be a dict of index tensors, got {type(category).__name__}")
        missing = [c for c in names if c not in category]
        if missing:
            raise KeyError(f"MMoE.forward: category features missing: {missing}")
        idx = [ops.as_index(category[n], f"category[{n!r}]") for n in names]
        return names, idx

    @staticmethod
    def _linears(seq):
        return [m for m in seq if isinstance(m, nn.Linear)]

    def _build(self, dense, names, idx, pin=False):
        """The forward's one rk_mmoe_forward launch over these inputs as a common.Bound (pin: prepare()'s
        pinned weight images); the outputs are patched in per call."""
        if not self.fits():
            raise RuntimeError("MMoE: configuration outside rk_mmoe_forward's envelope (common.mmoe_fits)")
        B, dev = dense.shape[0], dense.device
        if any(t.dim() != 1 or t.shape[0] != B for t in idx):
            raise ValueError("MMoE.forward: every category feature must be a 1-D tensor of the batch's length")
        image = common.PACKED.pin if pin else common.PACKED
        segs = [ops.dense_segment(dense, self.num_dense_features, 0)]
        col = self.num_dense_features
        for n, i in zip(names, idx):
            emb = self.embeddings[n]
            segs.append(ops.table_segment(emb.weight, i, col))
            col += emb.embedding_dim
        stacks = [[(image(l.weight), l.bias, l.out_features, "relu") for l in self._linears(seq)]
                  for seq in self.experts]
        towers = [[(image(l.weight), l.bias, l.out_features, "relu") for l in self._linears(seq)]
                  for seq in self.towers]
        gate_w = self._gate_w(*[g.weight for g in self.gates])
        gate_b = self._gate_b(*[g.bias for g in self.gates])
        gate_image = image(gate_w)
        heads = [(o.weight, o.bias) for o in self.tower_outputs]
        args, keep = ops.mmoe_forward_args(segs, self.input_dim, B, stacks, gate_image, gate_b, len(self.task_names),
                                           towers, heads, dev)
        return common.bound([("rk_mmoe_forward", args)], B, (keep, stacks, towers, gate_w, gate_b, gate_image),
                            self._patch)

    @staticmethod
    def _patch(_ep, args, out):
        prob, logit = out
        args[ops.MMOE_LOGITS_SLOT], args[ops.MMOE_PROBS_SLOT] = logit.data_ptr(), prob.data_ptr()

    @staticmethod
    def _run(bound, out, stream):
        bound.patch(out)
        common.run_launches(bound.launches, stream)

    def _outputs(self, B, dev):
        return common.empty_rows(dev, 2, (B, len(self.task_names)))

    def prepare(self, dense, category):
        """An eval forward bound to these input tensors (as DCNModel.prepare): returns `run()` that
        recomputes the whole forward from the current contents of the inputs with one rk_mmoe_forward
        launch and returns the same (probabilities, logits) tensors each time.  Binds the current
        weights and pins their packed images: prepare again after changing them."""
        if self.training:
            raise RuntimeError("MMoE.prepare: eval mode only (call .eval() first)")
        dense = ops.as_f32(dense, "dense")
        names = list(self.embeddings)
        idx = [ops.bound_index(category[n], f"category[{n!r}]") for n in names]
        if dense.shape[0] == 0:
            raise ValueError("MMoE.prepare: empty batch")
        return common.prepared(self, self._build(dense, names, idx, pin=True), dense.device, (dense, category))

    def forward(self, dense, category):
        if not self.trainable:
            check_eval(self)  # train mode is opt-in (trainable=True)
        dense = ops.as_f32(dense, "dense")
        if dense.dim() != 2 or dense.shape[1] < self.num_dense_features:
            raise ValueError(f"MMoE.forward: dense must be [B, {self.num_dense_features}], got {tuple(dense.shape)}")
        names, idx = self._indices(category)
        B, dev = dense.shape[0], dense.device
        if B == 0 and not self.training:
            return common.empty_rows(dev, 2, (0, len(self.task_names)))
        if self.training:  # Dropout live, HIP backward (rankops.train); an empty batch: zero gradients
            if not self.fits():
                raise RuntimeError("MMoE: configuration outside rk_mmoe_forward's envelope (common.mmoe_fits)")
            if any(t.dim() != 1 or t.shape[0] != B for t in idx):
                raise ValueError("MMoE.forward: every category feature must be a 1-D tensor of the batch's length")
            grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
            return train.mmoe_train_forward(self, dense, names, idx, grad)
        stream = ops._lib.raw_stream(dev)
        if all(t is category[n] for t, n in zip(idx, names)):  # no converted copies: addresses are the caller's
            bound = common.EagerCalls.lookup(self, [dense] + idx, stream, lambda: self._build(dense, names, idx))
        else:
            bound = self._build(dense, names, idx)
        out = self._outputs(B, dev)
        self._run(bound, out, stream)
        return out


class _CallableModule(types.ModuleType):
    """`rankops.mmoe(x, experts, gates, towers=None)`: the op-level function under the module's name."""

    def __call__(self, *args, **kwargs):
        return ops.mmoe(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
