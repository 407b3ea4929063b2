"""PLE (Progressive Layered Extraction, Tang et al., RecSys 2020) on the rankops engine: the third model
of the reference README's multi-task list (ESMM, MMOE, PLE), one probability per task and row.

The reference's README lists the model; it has no script for it, so the definition is this one, in the
conventions of rankops.MMoE and the reference's DCN (algorithm/DCN/dcn.py):

`PLE(vocab_dir, num_levels=2, num_specific_experts=2, num_shared_experts=2, expert_hidden_units=(256, 128),
     tower_hidden_units=(64,), task_names=("read_comment", "like", "click_avatar"), dropout_rate=0.1, *,
     vocab_sizes=None, trainable=False, sparse_grad=False)`
`forward(dense [B, 16], category {6 x [B]}) -> (probabilities [B, K], logits [B, K])`, column k = task_names[k].

With L = num_levels, ms = num_specific_experts, mc = num_shared_experts, K tasks, x = cat[dense, embeddings]
(width 50) and x_k^{-1} = x_s^{-1} = x, level j = 0 .. L - 1 is, in eval mode (Dropout the identity):

    f_{k,i} = specific_experts[k][i](x_k^{j-1})   i < ms        f_{s,i} = shared_experts[i](x_s^{j-1})   i < mc
    g_k = softmax(gates[k](x_k^{j-1}))       over ms + mc columns: c < ms -> f_{k,c}, else f_{s,c-ms}
    x_k^j = sum_c g_k[c] * (that expert's output)                  c ascending
    g_s = softmax(shared_gate(x_s^{j-1}))    over K ms + mc columns: k ms + i -> f_{k,i}, K ms + i -> f_{s,i}
    x_s^j = sum_c g_s[c] * (that expert's output)                  c ascending

(the last level has no shared_gate and no x_s), then logit_k = tower_outputs[k](towers[k](x_k^{L-1})) and
prob_k = sigmoid(logit_k).  Every expert is Linear + ReLU (+ Dropout(p) when p > 0) per entry of
expert_hidden_units; level 0's experts read width 50, later levels the last width H.  With L = 1 and
ms = 0 this is MMoE with mc experts.

Modules are created in this order (it fixes the seeded values and the state_dict keys): embeddings
(DCNModel's ModuleDict exactly: a DCN or MMoE checkpoint's `embeddings.*` load, the same seed gives the same
tables), levels = ModuleList of L modules, each creating specific_experts (ModuleList[K] of ModuleList[ms] of
Sequential), shared_experts (ModuleList[mc]), gates (ModuleList[K] of Linear) and, except at the last level,
shared_gate (Linear); then towers and tower_outputs as in MMoE.

One launch, rk_ple_forward (csrc/ple.hip): the row gather, every level's gates, experts and mixtures, the
towers and the heads; nothing between the gather and the logits reaches HBM.  CPU tensors raise the engine's
"ROCm GPU" error, and a configuration outside the kernel's envelope (common.ple_fits) is an error, not a
fallback.

Training is opt-in, as rankops.MMoE's: `PLE(..., trainable=True)` in train mode returns (probabilities, logits)
attached to autograd (rankops.train._PLETrain): rk_ple_forward_train, the same kernel with Dropout live behind
every ReLU and the activations kept, then ops.ple_backward — the heads and towers as MMoE's, per level
rk_ple_mix_backward and the grouped Linear backwards, in a number of launches that depends on L, the depths
and ceil((K ms + mc) / 16) only — and the embedding gradients; under no_grad it runs the same forward and keeps
nothing; `sparse_grad=True` hands the tables sparse COO gradients (rankops.SparseAdam).  The default
(trainable=False) raises NotImplementedError in train mode, as before.  Neither flag adds, reorders or
re-initialises a parameter.  Dropout masks are the engine's counter hash: with NE = K ms + mc stacks per level
(task k's at k ms + i, the shared at K ms + i), De = len(expert_hidden_units), Dt = len(tower_hidden_units) and
(seed, slot) of the last forward (seed = model._dropout.seed, slot = model._dropout.counter - 1: the device
counter is advanced once per train forward), expert s of level j, layer l drew
`ops.dropout_mask(seed + (j * NE + s) * De + l, slot, B, n, p)` and tower k layer l
`ops.dropout_mask(seed + L * NE * De + k * Dt + l, slot, B, n, p)` (element b * n + c).

`rankops.ple(x, levels, towers=None, return_levels=False)` is the same kernel on plain tensors (ops.ple),
differentiable when an input requires grad; this module is callable so that `rankops.ple` is both the module
and that function.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import common, ops
from .multitask import DEFAULT_TASKS, MultiTask, _stack


class _LevelGates:
    """The packed images of one level's gate weights (each gate reads its own representation, so they
    cannot be stacked into one GEMM), all written by a single rk_mlp_pack_weights launch and cached on the
    weights' versions as common.PackedWeights caches one image: a version bump rewrites the images in
    place on the stream, unless a prepared forward pinned them (then the new version gets fresh images)."""

    def __init__(self):
        self._key = None
        self._images = None
        self._pinned = False

    def __call__(self, weights, pin=False):
        key = common._key(weights)
        if key != self._key:
            dev = weights[0].device
            same_place = (self._key is not None and key[0] == self._key[0]
                          and [k[0] for k in key[1:]] == [k[0] for k in self._key[1:]])
            if not (same_place and not self._pinned and not torch.cuda.is_current_stream_capturing()):
                self._images = [ops.mlp_image(w.shape[0], w.shape[1], dev) for w in weights]
                self._pinned = False
            ops.pack_mlp_weights([(w.detach(), img) for w, img in zip(weights, self._images)], ops._lib.raw_stream(dev))
            self._key = key
        if pin:
            self._pinned = True
        return self._images


class _Level(nn.Module):
    def __init__(self, in_dim, num_tasks, ms, mc, units, dropout_rate, last):
        super().__init__()
        self.specific_experts = nn.ModuleList(
            nn.ModuleList(_stack(in_dim, units, dropout_rate)[0] for _ in range(ms)) for _ in range(num_tasks))
        self.shared_experts = nn.ModuleList(_stack(in_dim, units, dropout_rate)[0] for _ in range(mc))
        self.gates = nn.ModuleList(nn.Linear(in_dim, ms + mc) for _ in range(num_tasks))
        if not last:
            self.shared_gate = nn.Linear(in_dim, num_tasks * ms + mc)

    def all_gates(self):
        return list(self.gates) + ([self.shared_gate] if hasattr(self, "shared_gate") else [])

    def stacks(self):
        """The level's experts in the kernel's order: task k's at k ms + i, then the shared ones."""
        return [e for task in self.specific_experts for e in task] + list(self.shared_experts)


class PLE(MultiTask):
    NAME, ENTRY = "PLE", "rk_ple_forward"
    LOGITS_SLOT, PROBS_SLOT = ops.PLE_LOGITS_SLOT, ops.PLE_PROBS_SLOT

    def __init__(self, vocab_dir, num_levels=2, num_specific_experts=2, num_shared_experts=2,
                 expert_hidden_units=(256, 128), tower_hidden_units=(64,), task_names=DEFAULT_TASKS, dropout_rate=0.1,
                 *, vocab_sizes=None, trainable=False, sparse_grad=False):
        if int(num_levels) <= 0:
            raise ValueError(f"num_levels must be positive, got {num_levels!r}")
        if int(num_specific_experts) < 0 or int(num_shared_experts) <= 0:
            raise ValueError(f"num_specific_experts must be >= 0 and num_shared_experts >= 1, got "
                             f"{num_specific_experts!r}, {num_shared_experts!r}")
        super().__init__(vocab_dir, expert_hidden_units, tower_hidden_units, task_names, dropout_rate, vocab_sizes)
        self.trainable = bool(trainable)      # train mode runs the HIP train forward / backward (rankops.train)
        self.sparse_grad = bool(sparse_grad)  # train mode: tables get sparse COO gradients (rankops.SparseAdam)
        self.num_levels = int(num_levels)
        self.num_specific_experts = int(num_specific_experts)
        self.num_shared_experts = int(num_shared_experts)
        K, H = len(self.task_names), self.expert_hidden_units[-1]
        self.levels = nn.ModuleList(
            _Level(self.input_dim if j == 0 else H, K, self.num_specific_experts, self.num_shared_experts,
                   self.expert_hidden_units, self.dropout_rate, j == self.num_levels - 1)
            for j in range(self.num_levels))
        self._make_towers(H)
        self._gate_images = [_LevelGates() for _ in range(self.num_levels)]

    def fits(self) -> bool:
        return common.ple_fits(self.input_dim, 1 + len(self.embeddings), self.num_levels, len(self.task_names),
                               self.num_specific_experts, self.num_shared_experts, self.expert_hidden_units,
                               self.tower_hidden_units)

    def _launch_args(self, segs, B, dev, image, pin):
        K = len(self.task_names)
        experts, gates = [], []
        for level, packer in zip(self.levels, self._gate_images):
            experts += [(image(l.weight), l.bias) for seq in level.stacks() for l in self._linears(seq)]
            lin = level.all_gates()
            images = packer([g.weight for g in lin], pin)  # the level's K (+ 1) gate images, one pack launch
            gates += [(img, g.bias) for img, g in zip(images, lin)]
            if len(lin) == K:  # the last level: the shared gate's slot is never read
                gates.append((images[0], None))
        towers = [(image(l.weight), l.bias) for seq in self.towers for l in self._linears(seq)]
        heads = [(o.weight, o.bias) for o in self.tower_outputs]
        entries = experts + gates + towers + heads
        return ops.ple_forward_args(segs, self.input_dim, B, self.num_levels, K, self.num_specific_experts,
                                    self.num_shared_experts, self.expert_hidden_units, self.tower_hidden_units,
                                    entries, True, dev)


common.callable_module(__name__, ops.ple)  # rankops.ple(x, levels, towers=None, return_levels=False)
