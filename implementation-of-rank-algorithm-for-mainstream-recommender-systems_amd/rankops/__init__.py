"""rankops — MI355X-native CTR feature-interaction engine.

Drop-in `nn.Module`s for the reference's ranking models whose eval forward runs on
hand-written HIP kernels (gfx950) through the C ABI in include/rankops.h:

    DCNModel, cross_layer                  algorithm/DCN/dcn.py
    DeepFM                                 algorithm/DeepFM/deepfm.py
    DIN, Dice, din_attention               algorithm/DIN/din.py
    DIEN, dien_interest, dien_aux_loss     algorithm/DIEN/dien.py (with the auxiliary loss)
    dien_extract, dien_evolve, DIEN.score  the same split for one history and many candidates
    DIEN.forward / DIEN.prepare            the whole eval forward in one launch (rk_dien_forward), bound to
                                           its inputs by prepare() as DIN.prepare does
    AFM, create_feature_columns            algorithm/AFM/afm.py
    DeepCrossingModel, residual_unit       algorithm/DeepCrossing/deepcrossing.py
    BSTModel, BSTTransformer               algorithm/BST/bst.py
    FwFM                                   algorithm/FwFM/fwfm.py
    XDeepFM, cin                           xDeepFM (listed in the reference's README, no script in the
                                           snapshot): DeepFM with the Compressed Interaction Network,
                                           rk_cin_forward + the deep tail; trainable=True trains
                                           (rk_cin_backward, rk_cin_wgrad), cin is differentiable
    MMoE, mmoe                             MMoE, the base of the README's multi-task list (no script in the
                                           snapshot): one probability per task, the whole eval forward in
                                           one launch (rk_mmoe_forward); rankops.mmoe is the module and,
                                           called, the same kernel on plain tensors
    PLE, ple                               PLE, progressive layered extraction (the multi-task list's third
                                           model, no script in the reference): L levels of task and shared
                                           experts and gates, the whole eval forward in one launch
                                           (rk_ple_forward); rankops.ple is the module and, called, the op;
                                           trainable=True trains (rk_ple_forward_train, rk_ple_mix_backward
                                           and the grouped Linear backwards), ple is differentiable
    ESMM, esmm, esmm_loss                  ESMM, the entire space multi-task model (the multi-task list's
                                           first model, no script in the reference): towers over one gathered
                                           row, probabilities multiplied along the chain of events, the
                                           whole eval forward in one launch (rk_esmm_forward); rankops.esmm
                                           is the module and, called, the op; trainable=True trains
                                           (rk_esmm_forward_train, rk_esmm_joint_backward and the grouped
                                           Linear backwards); esmm_loss is the entire-space loss in the log
                                           domain with its analytic gradient (rk_esmm_loss)

    FiBiNET, fibinet_interaction           FiBiNET (listed in the reference's README, no script in the
                                           snapshot): SENET field attention and the bilinear interaction,
                                           the whole eval forward in one launch (rk_fibinet_forward);
                                           fibinet_interaction is the interaction alone on plain tensors
                                           (rk_fibinet_interaction); eval only

`rankops.sharded.ShardedDeepFM` adds the table-sharded multi-GPU DeepFM lookup (RCCL
all-to-all); `rankops.loader` (Vocabulary, BatchAssembler, wechat_vocabularies) replaces the
reference's Dataset bucketing + collate with C++ column bucketing and one H2D copy per batch;
`rankops.metrics` (EvalAccumulator, roc_auc) computes evaluate()'s loss / accuracy / AUC on the GPU;
`rankops.ranking` (topk_segments, topk_per_request, grouped_auc; DIEN.rank) keeps the best k candidates
of each request and computes the per-user AUC / GAUC there too;
`rankops.train` holds the HIP backward (train-mode forwards return autograd-connected outputs)
and `rankops.Adam`, a one-launch torch.optim.Adam; with `sparse_grad=True` a model's tables get
sparse gradients and `rankops.SparseAdam` (torch.optim.SparseAdam / LazyAdam) updates only their rows.
Import order matters: torch first, so librankops binds to torch's HIP runtime.
"""
import torch  # noqa: F401

from ._lib import RankOpsError, error_flags, load as load_library  # noqa: F401
from .afm import AFM, create_feature_columns  # noqa: F401
from .bst import BSTModel, BSTTransformer  # noqa: F401
from .dcn import DCNModel, cross_layer  # noqa: F401
from .deepcrossing import DeepCrossingModel, residual_unit  # noqa: F401
from .deepfm import DeepFM  # noqa: F401
from .din import DIN, Dice, din_attention, din_attention_gather  # noqa: F401
from .dien import (DIEN, DIENInterests, dien_aux_loss, dien_aux_loss_gather, dien_evolve, dien_extract,  # noqa: F401
                   dien_extract_gather, dien_interest, dien_interest_gather)
from .fibinet import FiBiNET  # noqa: F401
from .fwfm import FwFM  # noqa: F401
from .loader import BatchAssembler, Vocabulary, label_encode, wechat_vocabularies  # noqa: F401
from . import mmoe  # noqa: F401  (callable: rankops.mmoe(x, experts, gates, towers=None))
from .mmoe import MMoE  # noqa: F401
from . import ple  # noqa: F401  (callable: rankops.ple(x, levels, towers=None, return_levels=False))
from .ple import PLE  # noqa: F401
from . import esmm  # noqa: F401  (callable: rankops.esmm(x, towers, return_conditional=False))
from .esmm import ESMM  # noqa: F401
from .ops import esmm_loss  # noqa: F401
from .metrics import EvalAccumulator, roc_auc  # noqa: F401
from .ranking import GroupedAUC, GroupTable, RequestTopK, grouped_auc, topk_per_request, topk_segments  # noqa: F401
from .ops import cin, fibinet_interaction  # noqa: F401
from .train import Adam, SparseAdam  # noqa: F401
from .xdeepfm import XDeepFM  # noqa: F401

__all__ = [
    "AFM", "BSTModel", "BSTTransformer", "BatchAssembler", "DCNModel", "DIN", "DeepCrossingModel", "DeepFM",
    "Dice", "FwFM", "RankOpsError", "Vocabulary", "create_feature_columns", "cross_layer", "din_attention", "din_attention_gather",
    "error_flags", "load_library", "residual_unit", "wechat_vocabularies", "EvalAccumulator", "roc_auc",
    "label_encode", "Adam", "DIEN", "dien_interest", "dien_interest_gather",
    "dien_aux_loss", "dien_aux_loss_gather", "dien_extract", "dien_extract_gather", "dien_evolve", "DIENInterests",
    "SparseAdam", "XDeepFM", "cin", "FiBiNET", "fibinet_interaction", "MMoE", "mmoe", "PLE", "ple", "ESMM", "esmm", "esmm_loss", "RequestTopK", "GroupedAUC", "GroupTable", "topk_segments", "topk_per_request", "grouped_auc",
]
