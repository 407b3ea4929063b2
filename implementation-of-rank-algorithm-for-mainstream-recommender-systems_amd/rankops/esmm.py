"""ESMM (Entire Space Multi-task Model, Ma et al., SIGIR 2018) on the rankops engine: the first entry of
the reference README's multi-task list (ESMM, MMOE, PLE).  Towers over shared embeddings, with
probabilities multiplied along a chain of events (impression -> click -> conversion), so that every
task is trained and evaluated over the entire space of impressions.

The reference's README lists the model; its script is not in the snapshot, so the definition is this
one, in rankops.MMoE's conventions:

`ESMM(vocab_dir, tower_hidden_units=(256, 128, 64), task_names=("click", "conversion"), dropout_rate=0.1, *,
      vocab_sizes=None, trainable=False, sparse_grad=False)`
`forward(dense [B, 16], category {6 x [B]}) -> (probabilities [B, K], logits [B, K])`, K = len(task_names) >= 2.

Modules are created in this order (it fixes the seeded values and the state_dict keys): embeddings
(MultiTask's ModuleDict exactly: a DCN, MMoE or PLE checkpoint's `embeddings.*` load, the same seed gives
the same tables), towers = ModuleList of K Sequential(Linear, ReLU, Dropout(p) per hidden unit; no Dropout
when p == 0) over the row, tower_outputs = ModuleList of K Linear(last_width, 1).  In eval mode (Dropout
the identity), with x = cat[dense, embeddings]:

    logit_k = tower_outputs[k](towers[k](x))          every tower reads the same x
    c_k     = sigmoid(logit_k)                         the conditional probability (pCTR, pCVR, ...)
    prob_k  = c_0 c_1 ... c_k   (k ascending)          the entire-space probability (pCTR, pCTCVR, ...)

K = 2 is the paper's model; a longer task_names gives the chain form.  `probabilities` holds what ESMM
is trained and evaluated on (one EvalAccumulator per task takes probs[:, k]); `logits` holds the
conditional logits: pCVR is sigmoid(logits[:, 1]).

One launch, rk_esmm_forward (csrc/esmm.hip): the row is gathered once for all towers and no tower
activation reaches HBM.  CPU tensors raise the engine's "ROCm GPU" error; a configuration outside the
kernel's envelope (common.esmm_fits: K in 2..8, 1..3 tower layers, widths <= 512) is an error, not a
fallback.

Training is opt-in, as for MMoE: `ESMM(..., trainable=True)` in train mode returns (probabilities, logits)
attached to autograd (rankops.train._ESMMTrain): rk_esmm_forward_train, the same kernel with Dropout live
behind every ReLU and the activations kept, then ops.esmm_backward (the fold of the probabilities'
gradients onto the logits, the heads, the towers grouped over the tasks, layer 0 of all towers as one
stacked product) and the embedding gradients, a number of launches that does not depend on K.
`rankops.esmm_loss(logits, labels)` is the loss to train it with: the entire-space BCE in the log domain
with an analytic gradient (rk_esmm_loss); BCE on the product of float32 sigmoids is wrong once logits
saturate.  `sparse_grad=True` hands the tables sparse COO gradients (rankops.SparseAdam).  The default
(trainable=False) raises NotImplementedError in train mode.  Neither flag adds, reorders or re-initialises
a parameter.  Dropout masks are the engine's counter hash: with Dt = len(tower_hidden_units) and
(seed, slot) of the forward (model._dropout), tower k layer l drew
`ops.dropout_mask(seed + k * Dt + l, slot, B, n, p)` (element b * n + j).

`rankops.esmm(x, towers, return_conditional=False)` is the same kernel on plain tensors (ops.esmm),
differentiable when an input requires grad; this module is callable so that `rankops.esmm` is both the
module and that function.
"""
from __future__ import annotations

from . import common, ops
from .multitask import MultiTask

DEFAULT_TASKS = ("click", "conversion")


class ESMM(MultiTask):
    NAME, ENTRY = "ESMM", "rk_esmm_forward"
    LOGITS_SLOT, PROBS_SLOT = ops.ESMM_LOGITS_SLOT, ops.ESMM_PROBS_SLOT

    def __init__(self, vocab_dir, tower_hidden_units=(256, 128, 64), task_names=DEFAULT_TASKS, dropout_rate=0.1, *,
                 vocab_sizes=None, trainable=False, sparse_grad=False):
        tower_hidden_units = tuple(tower_hidden_units)
        task_names = tuple(task_names)
        if len(tower_hidden_units) == 0:
            raise ValueError("tower_hidden_units must be a non-empty list of positive widths, got ()")
        if len(task_names) < 2:
            raise ValueError(f"task_names must name at least two events of the chain, got {task_names!r}")
        super().__init__(vocab_dir, None, tower_hidden_units, task_names, dropout_rate, vocab_sizes)
        self.trainable = bool(trainable)      # train mode runs the HIP train forward / backward (rankops.train)
        self.sparse_grad = bool(sparse_grad)  # train mode: tables get sparse COO gradients (rankops.SparseAdam)
        self._make_towers(self.input_dim)

    def fits(self) -> bool:
        return common.esmm_fits(self.input_dim, 1 + len(self.embeddings), len(self.task_names),
                                self.tower_hidden_units)

    def _launch_args(self, segs, B, dev, image, pin):
        towers = [[(image(l.weight), l.bias, l.out_features, "relu") for l in self._linears(seq)]
                  for seq in self.towers]
        heads = [(o.weight, o.bias) for o in self.tower_outputs]
        args, keep = ops.esmm_forward_args(segs, self.input_dim, B, towers, heads, dev)
        return args, (keep, towers)


common.callable_module(__name__, ops.esmm)  # rankops.esmm(x, towers, return_conditional=False)
