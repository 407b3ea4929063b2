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

import torch.nn as nn

from . import common, ops
from .multitask import DEFAULT_TASKS, MultiTask, _stack


class MMoE(MultiTask):
    NAME, ENTRY = "MMoE", "rk_mmoe_forward"
    LOGITS_SLOT, PROBS_SLOT = ops.MMOE_LOGITS_SLOT, ops.MMOE_PROBS_SLOT

    def __init__(self, vocab_dir, num_experts=4, expert_hidden_units=(256, 128), tower_hidden_units=(64,),
                 task_names=DEFAULT_TASKS, dropout_rate=0.1, *, vocab_sizes=None, trainable=False, sparse_grad=False):
        if int(num_experts) <= 0:
            raise ValueError(f"num_experts must be positive, got {num_experts!r}")
        super().__init__(vocab_dir, expert_hidden_units, tower_hidden_units, task_names, dropout_rate, vocab_sizes)
        self.trainable = bool(trainable)      # train mode runs the HIP train forward / backward (rankops.train)
        self.sparse_grad = bool(sparse_grad)  # train mode: tables get sparse COO gradients (rankops.SparseAdam)
        self.num_experts = int(num_experts)
        self.experts = nn.ModuleList()
        for _ in range(self.num_experts):
            seq, width = _stack(self.input_dim, self.expert_hidden_units, self.dropout_rate)
            self.experts.append(seq)
        self.gates = nn.ModuleList(nn.Linear(self.input_dim, self.num_experts) for _ in self.task_names)
        self._make_towers(width)
        self._gate_w, self._gate_b = common.Packed(), common.Packed()  # the K gates stacked to [K E, width]

    def fits(self) -> bool:
        return common.mmoe_fits(self.input_dim, 1 + len(self.embeddings), self.num_experts, len(self.task_names),
                                self.expert_hidden_units, self.tower_hidden_units)

    def _launch_args(self, segs, B, dev, image, pin):
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
        return args, (keep, stacks, towers, gate_w, gate_b, gate_image)


common.callable_module(__name__, ops.mmoe)  # rankops.mmoe(x, experts, gates, towers=None)
