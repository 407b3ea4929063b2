"""FwFM (field-weighted factorization machine) on the rankops engine — drop-in for
algorithm/FwFM/fwfm.py.

`FwFM(field_dims, embed_dim)` keeps the reference constructor, parameter creation order (so a
seeded construction draws the same weights) and state_dict keys (`linear.<f>.weight`,
`embedding.<f>.weight`, `field_weight`, `bias`; fwfm.py:87-112), and
`forward(x) -> sigmoid(y).squeeze(1)` over `x = {'userid', 'feedid', 'device', 'authorid',
'bgm_song_id', 'bgm_singer_id'}` int64 index tensors (fwfm.py:114-139).  Tables have
`len(vocab)` rows (no +1, fwfm.py:235-242); the indices come from the dataset-level
LabelEncoder bucketing in `rankops.loader.label_encode` (fwfm.py:48-67).

The whole forward — 12 gathers, the 15 weighted pair dots, the linear term, bias and sigmoid — is
one rk_fwfm_forward launch.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import common, ops, train
from .common import EngineModule, check_eval

FWFM_FIELDS = ("userid", "feedid", "device", "authorid", "bgm_song_id", "bgm_singer_id")


class FwFM(EngineModule):
    def __init__(self, field_dims, embed_dim, *, field_names=FWFM_FIELDS, sparse_grad=False):
        super().__init__()
        self.sparse_grad = bool(sparse_grad)  # train mode: tables get sparse COO gradients (rankops.SparseAdam)
        self.field_dims = field_dims
        self.num_fields = len(field_dims)
        self.embed_dim = embed_dim
        if len(field_names) != self.num_fields:
            raise ValueError(f"FwFM: {self.num_fields} field_dims but {len(field_names)} field names")
        self.field_names = tuple(field_names)
        self.linear = nn.ModuleList([nn.Embedding(n, 1) for n in field_dims])
        self.embedding = nn.ModuleList([nn.Embedding(n, embed_dim) for n in field_dims])
        for emb in self.embedding:
            nn.init.xavier_uniform_(emb.weight)
        self.num_pairs = self.num_fields * (self.num_fields - 1) // 2
        self.field_weight = nn.Parameter(torch.randn(self.num_pairs), requires_grad=True)
        self.bias = nn.Parameter(torch.zeros(1))

    def _build(self, idx):
        """The forward's one rk_fwfm_forward launch bound to the int64 [B] index tensors `idx` (field
        order) as a common.Bound; the outputs are patched in per call.  The launch reads the
        parameters in place."""
        B, dev = idx[0].shape[0], idx[0].device
        emb = [ops.table_segment(self.embedding[f].weight, t, 0) for f, t in enumerate(idx)]
        lin = [ops.table_segment(self.linear[f].weight, t, 0) for f, t in enumerate(idx)]
        fw, bias = ops.as_f32(self.field_weight, "field_weight"), ops.as_f32(self.bias, "bias")
        args = ops.fwfm_forward_args(emb, lin, self.embed_dim, B, fw, bias, None, None)
        return common.bound([("rk_fwfm_forward", args)], B, (fw, bias), self._patch)

    @staticmethod
    def _patch(_ep, args, out):
        prob, logit = out
        args[ops.FWFM_LOGIT_SLOT], args[ops.FWFM_PROB_SLOT] = ops.ptr(logit), prob.data_ptr()

    @staticmethod
    def _outputs(B, dev, return_logit=True):
        prob = torch.empty(B, device=dev, dtype=torch.float32)
        return prob, (torch.empty(B, device=dev, dtype=torch.float32) if return_logit else None)

    def prepare(self, x):
        """An eval forward bound to these index tensors (as DCNModel.prepare): returns `run()` that
        recomputes (prob, logit) [B] from the indices' current contents with one rk_fwfm_forward
        launch, into the same tensors each time.  The launch reads the parameters in place.  Index
        tensors must be int64 (bound by address, never copied)."""
        if self.training:
            raise RuntimeError("FwFM.prepare: eval mode only (call .eval() first)")
        idxs = [ops.bound_index(x[name], f"x[{name!r}]") for name in self.field_names]
        return common.prepared(self, self._build(idxs), idxs[0].device, x)

    def forward(self, x, *, return_logit=False):
        """x: {field: int64 [B]} -> probabilities [B] (and the logits [B] with return_logit).
        Under .train() with autograd on, the probabilities carry the HIP backward (rankops.train)."""
        first = x.get(self.field_names[0], None) if isinstance(x, dict) else None
        if not self.training and isinstance(first, torch.Tensor) and first.shape[0] == 0:
            prob, logit = common.empty_rows(ops.require_gpu(first, "x").device, 2, shape=(0,))
            return (prob, logit) if return_logit else prob
        bound = None
        if not self.training:
            try:
                idxs = [x[n] for n in self.field_names]
            except (KeyError, TypeError):
                idxs = ()
            # the caller's own int64 [B] tensors: the cached launch (anything else: the checks below)
            if idxs and all(isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.dim() == 1 for t in idxs) \
                    and idxs[0].device.type == "cuda" and all(t.shape == idxs[0].shape for t in idxs):
                bound = common.EagerCalls.lookup(self, idxs, ops._lib.raw_stream(idxs[0].device),
                                                 lambda: self._build(idxs))
        if self.training and not (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            check_eval(self)  # a train-mode forward without autograd is not implemented
        if bound is None:
            B = ops.as_index(x[self.field_names[0]], f"x[{self.field_names[0]!r}]").shape[0]
            idxs = []
            for name in self.field_names:
                idx = ops.as_index(x[name], f"x[{name!r}]")
                if idx.shape != (B,):
                    raise ValueError(f"FwFM.forward: x[{name!r}] has shape {tuple(idx.shape)}, expected ({B},)")
                idxs.append(idx)
            if self.training:  # the train Function marshals its own segments
                return train.fwfm_train_forward(self, idxs, return_logit)
            bound = self._build(idxs)
        dev = idxs[0].device
        out = self._outputs(bound.batch, dev, return_logit)
        bound.patch(out)
        common.run_launches(bound.launches, ops._lib.raw_stream(dev))
        return out if return_logit else out[0]
