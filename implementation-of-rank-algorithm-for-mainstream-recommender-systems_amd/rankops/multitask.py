"""What the multi-task models (rankops.MMoE, rankops.PLE, rankops.ESMM) share: the inputs of the reference's DCN
(16 dense columns and six embedding tables, width 50), K towers with one head each, and an eval forward
that is one launch returning (probabilities [B, K], logits [B, K]).

A model supplies NAME (its name in messages), ENTRY (the C entry point of that launch) and
LOGITS_SLOT / PROBS_SLOT (the two outputs' positions in its argument list), `fits()`, and
`_launch_args(segs, B, dev, image, pin)`, the launch's argument list over the row segments `segs` with
what it must keep alive.  Training is opt-in per instance (`trainable`, `sparse_grad`, set by the model's
constructor): train mode then runs rankops.train.multitask_train_forward, which finds the model's train
forward, autograd function and parameter list by NAME.  Its __init__ calls this one first (embeddings are the first modules created),
then creates its experts and gates, then calls `_make_towers`.  A model without experts (ESMM) passes
expert_hidden_units=None and builds its towers over the row.
"""
from __future__ import annotations

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


class MultiTask(EngineModule):
    NAME = ENTRY = LOGITS_SLOT = PROBS_SLOT = None
    trainable = sparse_grad = False

    def __init__(self, vocab_dir, expert_hidden_units, tower_hidden_units, task_names, dropout_rate, vocab_sizes):
        super().__init__()
        self.dropout_rate = float(dropout_rate)
        no_experts = expert_hidden_units is None  # (ESMM: the towers stand on the row itself)
        expert_hidden_units = () if no_experts else tuple(int(h) for h in expert_hidden_units)
        tower_hidden_units = tuple(int(h) for h in tower_hidden_units)
        task_names = tuple(task_names)
        if (not no_experts and len(expert_hidden_units) == 0) or any(
                h <= 0 for h in expert_hidden_units + tower_hidden_units):
            raise ValueError(f"expert_hidden_units must be a non-empty list of positive widths and tower_hidden_units "
                             f"a list of positive widths, got {expert_hidden_units!r}, {tower_hidden_units!r}")
        if len(task_names) == 0 or len(set(task_names)) != len(task_names):
            raise ValueError(f"task_names must be a non-empty list of distinct names, got {task_names!r}")
        if not 0 <= dropout_rate < 1:
            raise ValueError(f"dropout_rate must lie in [0, 1), got {dropout_rate!r}")
        fields = ("userid", "feedid", "device", "authorid", "bgm_song_id", "bgm_singer_id", "manual_tag_list")
        self.vocab_sizes = {f: table_rows(vocab_dir, f, vocab_sizes) for f in fields}
        self.num_dense_features = 16
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

    def _make_towers(self, width):
        """towers and tower_outputs over the tasks' mixtures of `width` columns."""
        K = len(self.task_names)
        self.towers = nn.ModuleList()
        last = width
        for _ in range(K):
            seq, last = _stack(width, self.tower_hidden_units, self.dropout_rate)
            self.towers.append(seq)
        self.tower_outputs = nn.ModuleList(nn.Linear(last, 1) for _ in range(K))

    def _inputs(self, dense, category):
        dense = ops.as_f32(dense, "dense")
        if dense.dim() != 2 or dense.shape[1] < self.num_dense_features:
            raise ValueError(f"{self.NAME}.forward: dense must be [B, {self.num_dense_features}], got {tuple(dense.shape)}")
        return (dense,) + self._indices(category)

    def _indices(self, category):
        names = list(self.embeddings)
        if not isinstance(category, dict):
            raise TypeError(f"{self.NAME}.forward: category must be a dict of index tensors, got {type(category).__name__}")
        missing = [c for c in names if c not in category]
        if missing:
            raise KeyError(f"{self.NAME}.forward: category features missing: {missing}")
        idx = [ops.as_index(category[n], f"category[{n!r}]") for n in names]
        return names, idx

    @staticmethod
    def _linears(seq):
        return [m for m in seq if isinstance(m, nn.Linear)]

    def _check(self, B, idx):
        if not self.fits():
            raise RuntimeError(f"{self.NAME}: configuration outside {self.ENTRY}'s envelope "
                               f"(common.{self.NAME.lower()}_fits)")
        if any(t.dim() != 1 or t.shape[0] != B for t in idx):
            raise ValueError(f"{self.NAME}.forward: every category feature must be a 1-D tensor of the batch's length")

    def _segments(self, dense, names, idx):
        """The gathered row: the dense columns, then each table's row at the sample's index."""
        segs = [ops.dense_segment(dense, self.num_dense_features, 0)]
        col = self.num_dense_features
        for n, i in zip(names, idx):
            emb = self.embeddings[n]
            segs.append(ops.table_segment(emb.weight, i, col))
            col += emb.embedding_dim
        return segs

    def _build(self, dense, names, idx, pin=False):
        """The forward's one launch over these inputs as a common.Bound (pin: prepare()'s pinned weight
        images); the outputs are patched in per call."""
        B, dev = dense.shape[0], dense.device
        self._check(B, idx)
        image = common.PACKED.pin if pin else common.PACKED
        args, keep = self._launch_args(self._segments(dense, names, idx), B, dev, image, pin)
        return common.bound([(self.ENTRY, args)], B, keep, self._patch)

    @classmethod
    def _patch(cls, _ep, args, out):
        prob, logit = out
        args[cls.LOGITS_SLOT], args[cls.PROBS_SLOT] = logit.data_ptr(), prob.data_ptr()

    @staticmethod
    def _run(bound, out, stream):
        bound.patch(out)
        common.run_launches(bound.launches, stream)

    def _outputs(self, B, dev):
        return common.empty_rows(dev, 2, (B, len(self.task_names)))

    def prepare(self, dense, category):
        """An eval forward bound to these input tensors (as DCNModel.prepare): returns `run()` that
        recomputes the whole forward from the current contents of the inputs with one launch and returns
        the same (probabilities, logits) tensors each time.  Binds the current weights and pins their
        packed images: prepare again after changing them."""
        if self.training:
            raise RuntimeError(f"{self.NAME}.prepare: eval mode only (call .eval() first)")
        dense = ops.as_f32(dense, "dense")
        names = list(self.embeddings)
        idx = [ops.bound_index(category[n], f"category[{n!r}]") for n in names]
        if dense.shape[0] == 0:
            raise ValueError(f"{self.NAME}.prepare: empty batch")
        return common.prepared(self, self._build(dense, names, idx, pin=True), dense.device, (dense, category))

    def _eval_forward(self, dense, names, idx, category):
        B, dev = dense.shape[0], dense.device
        if B == 0:
            return common.empty_rows(dev, 2, (0, len(self.task_names)))
        stream = ops._lib.raw_stream(dev)
        if all(t is category[n] for t, n in zip(idx, names)):  # no converted copies: addresses are the caller's
            bound = common.EagerCalls.lookup(self, [dense] + idx, stream, lambda: self._build(dense, names, idx))
        else:
            bound = self._build(dense, names, idx)
        out = self._outputs(B, dev)
        self._run(bound, out, stream)
        return out

    def forward(self, dense, category):
        if not self.trainable:
            check_eval(self)  # train mode is opt-in (trainable=True)
        dense, names, idx = self._inputs(dense, category)
        if self.training:  # Dropout live, HIP backward (rankops.train); an empty batch: zero gradients
            self._check(dense.shape[0], idx)
            grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
            return train.multitask_train_forward(self, dense, names, idx, grad)
        return self._eval_forward(dense, names, idx, category)
