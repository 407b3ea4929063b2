"""DIEN (Deep Interest Evolution Network) on the rankops engine — the model of algorithm/DIEN/dien.py
(a TF1 Estimator there; it does not run, so this is its mathematics, not a line-for-line port).

`DIEN(vocab_dir, hidden_units=None, activation='dice', dropout_rate=0.1, batch_norm=True,
custom_gru_type='AGRU', gru_output_units=8)` takes the reference's flags (dien.py:40-53) and
`forward(dense, category, sequence, target) -> (probability, logit)` the input dictionaries of
`rankops.DIN`.  Eval mode only: train mode raises (common.check_eval); the auxiliary loss is left
out (the reference says it does not run, dien.py:256-300).

Parameters: `embeddings.*` as in DIN except that target and history share the one `feedid` table
(shared_embedding_columns, dien.py:126); `gru.gates` / `gru.candidate` (TF GRUCell: Linear(H+nh, 2nh)
with the reset rows first, Linear(H+nh, nh)); `attention_project_matrix` [nh, H];
`evolution.gates` / `evolution.candidate` (AGRU / AUGRU cell: Linear(2nh, 2nh), Linear(2nh, nh));
`fcn.*`, `output_layer.*` as in DIN.  Initialisation as TF does it: Glorot-uniform kernels, gate
biases 1 (custom_grucell.py:66-68), other biases 0.

Launches: rk_concat_gather builds [dense | category | target | .] in one row buffer,
rk_dien_interest (history gather, GRU, attention scores, masked softmax, AGRU / AUGRU) writes the
final interest state into the row's last nh columns, and the fcn stack runs as DIN's tail.  The row
order is DIN's (dense in the given order, category in ModuleDict order), not input_layer's
alphabetical one: there is no TF checkpoint this could ever load.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import common, ops
from .common import EngineModule, Layer, check_eval, load_vocabulary, run_tail, table_rows
from .din import FIELDS, SEQ_KEY, Dice

ENVELOPE = "H (embedding width) in {8, 16, 32}, nh (gru_output_units) in {8, 16}, 1 <= T <= 256"
WEIGHT_NAMES = ("Wg", "bg", "Wc", "bc", "A", "Vg", "vg", "Vc", "vc")


def _cell(cell_type) -> int:
    if cell_type not in ops.DIEN_CELLS:
        raise ValueError(f"rankops DIEN: custom_gru_type must be 'AGRU' or 'AUGRU', got {cell_type!r}")
    return ops.DIEN_CELLS[cell_type]


def _check_envelope(H: int, nh: int, T: int):
    if H not in (8, 16, 32) or nh not in (8, 16) or not 1 <= T <= 256:
        raise NotImplementedError(f"rankops dien_interest: H={H}, nh={nh}, T={T} is outside the kernel's envelope: "
                                  f"{ENVELOPE}")


def _weights(weights, H: int):
    """(Wg, bg, Wc, bc, A, Vg, vg, Vc, vc) checked against H and each other; returns them
    contiguous with nh."""
    if len(weights) != 9:
        raise ValueError(f"rankops dien_interest: weights must be {WEIGHT_NAMES}, got {len(weights)} tensors")
    ws = [ops.as_f32(w, f"weights[{n}]").contiguous() for n, w in zip(WEIGHT_NAMES, weights)]
    if ws[4].dim() != 2 or ws[4].shape[1] != H:
        raise ValueError(f"rankops dien_interest: A must be [nh, {H}], got {tuple(ws[4].shape)}")
    nh = ws[4].shape[0]
    want = ((2 * nh, H + nh), (2 * nh,), (nh, H + nh), (nh,), (nh, H), (2 * nh, 2 * nh), (2 * nh,), (nh, 2 * nh),
            (nh,))
    for n, w, shape in zip(WEIGHT_NAMES, ws, want):
        if tuple(w.shape) != shape:
            raise ValueError(f"rankops dien_interest: {n} must be {shape}, got {tuple(w.shape)}")
    return ws, nh


def _convert(rc_error, H, nh, T):
    if getattr(rc_error, "code", None) == ops._lib.RK_ERR_UNSUPPORTED:
        raise NotImplementedError(f"rankops dien_interest: H={H}, nh={nh}, T={T}: {rc_error}; envelope: "
                                  f"{ENVELOPE}") from rc_error
    raise rc_error


def dien_interest(query, keys, keys_length, weights, cell_type="AGRU", return_attention=False):
    """dien_interest(query[B,H], keys[B,T,H], keys_length[B], weights) -> final interest state [B,nh]
    (dien.py:198-229) on rk_dien_interest_dense: TF GRUCell over the keys, attention of the hidden
    states against `A . query` (softmax over all T positions, positions t >= keys_length masked
    with -2^32+1), then the AGRU / AUGRU cell over the hidden states for t < keys_length.
    `weights` = (Wg, bg, Wc, bc, A, Vg, vg, Vc, vc) device tensors (rankops.h);
    `return_attention` adds the attention weights [B,T]."""
    cell = _cell(cell_type)
    query = ops.as_f32(query, "query")
    keys = ops.as_f32(keys, "keys")
    keys_length = ops.as_index(keys_length, "keys_length")
    if keys.dim() != 3 or query.dim() != 2 or query.shape[0] != keys.shape[0] or query.shape[1] != keys.shape[2]:
        raise ValueError(f"dien_interest: query {tuple(query.shape)} and keys {tuple(keys.shape)} do not match")
    B, T, H = keys.shape
    if keys_length.dim() != 1 or keys_length.shape[0] != B:
        raise ValueError(f"dien_interest: keys_length must be [{B}], got {tuple(keys_length.shape)}")
    ws, nh = _weights(weights, H)
    _check_envelope(H, nh, T)
    if keys.stride(2) != 1 or keys.stride(1) % 4 or keys.stride(0) % 4 or keys.data_ptr() % 16:
        keys = keys.contiguous()
    if query.stride(1) != 1:
        query = query.contiguous()
    out = torch.empty(B, nh, device=keys.device, dtype=torch.float32)
    att = torch.empty(B, T, device=keys.device, dtype=torch.float32) if return_attention else None
    if B > 0:
        try:
            ops.dien_interest_dense(query, keys, keys_length.contiguous(), nh, cell, ws, out, att)
        except ops._lib.RankOpsError as e:
            _convert(e, H, nh, T)
    return (out, att) if return_attention else out


def dien_interest_gather(query, table, seq, keys_length, weights, cell_type="AGRU", return_attention=False):
    """dien_interest with the history given as (embedding table [V,H], ids [B,T]): the gather
    happens inside the kernel (rk_dien_interest); ids at t >= keys_length are never read."""
    cell = _cell(cell_type)
    query = ops.as_f32(query, "query")
    table = ops.as_f32(table, "table")
    seq = ops.as_index(seq, "keys index")
    keys_length = ops.as_index(keys_length, "keys_length")
    if query.dim() != 2 or table.dim() != 2 or seq.dim() != 2 or table.shape[1] != query.shape[1] \
            or seq.shape[0] != query.shape[0]:
        raise ValueError(f"dien_interest_gather: query {tuple(query.shape)}, table {tuple(table.shape)} and ids "
                         f"{tuple(seq.shape)} do not match")
    B, H = query.shape
    T = seq.shape[1]
    if keys_length.dim() != 1 or keys_length.shape[0] != B:
        raise ValueError(f"dien_interest_gather: keys_length must be [{B}], got {tuple(keys_length.shape)}")
    ws, nh = _weights(weights, H)
    _check_envelope(H, nh, T)
    if table.stride(1) != 1 or table.stride(0) % 4 or table.data_ptr() % 16:
        table = table.contiguous()
    if query.stride(1) != 1:
        query = query.contiguous()
    out = torch.empty(B, nh, device=query.device, dtype=torch.float32)
    att = torch.empty(B, T, device=query.device, dtype=torch.float32) if return_attention else None
    if B > 0:
        try:
            ops.dien_interest(query.data_ptr(), query.stride(0), table, seq.contiguous(), keys_length.contiguous(), T,
                              H, nh, cell, ws, out.data_ptr(), out.stride(0), att, B, query.device)
        except ops._lib.RankOpsError as e:
            _convert(e, H, nh, T)
    return (out, att) if return_attention else out


def _tf_linear(in_features: int, out_features: int, bias_value: float = 0.0) -> nn.Linear:
    """nn.Linear initialised as a TF dense / _Linear layer: Glorot-uniform kernel, constant bias."""
    lin = nn.Linear(in_features, out_features)
    nn.init.xavier_uniform_(lin.weight)
    nn.init.constant_(lin.bias, bias_value)
    return lin


class DIEN(EngineModule):
    def __init__(self, vocab_dir, hidden_units=None, activation='dice', dropout_rate=0.1, batch_norm=True,
                 custom_gru_type='AGRU', gru_output_units=8, *, vocab_sizes=None, embedding_dim=16):
        super().__init__()
        if hidden_units is None:
            hidden_units = [512, 256, 128]
        _cell(custom_gru_type)
        self.activation = activation
        self.dropout_rate = dropout_rate
        self.batch_norm = batch_norm
        self.custom_gru_type = custom_gru_type
        self.gru_output_units = nh = gru_output_units
        self.vocab_sizes = {f: table_rows(vocab_dir, f, vocab_sizes) for f in FIELDS}
        self.num_dense_features = 16
        # target and history share the feedid table (shared_embedding_columns, dien.py:126)
        self.embeddings = nn.ModuleDict({
            "userid": nn.Embedding(self.vocab_sizes["userid"], 16),
            "device": nn.Embedding(self.vocab_sizes["device"], 2),
            "authorid": nn.Embedding(self.vocab_sizes["authorid"], 4),
            "bgm_song_id": nn.Embedding(self.vocab_sizes["bgm_song_id"], 4),
            "bgm_singer_id": nn.Embedding(self.vocab_sizes["bgm_singer_id"], 4),
            "manual_tag_list": nn.Embedding(self.vocab_sizes["manual_tag_list"], 4),
            "feedid": nn.Embedding(self.vocab_sizes["feedid"], embedding_dim),
        })
        H = embedding_dim
        self.gru = nn.ModuleDict({"gates": _tf_linear(H + nh, 2 * nh, 1.0), "candidate": _tf_linear(H + nh, nh)})
        self.attention_project_matrix = nn.Parameter(nn.init.xavier_uniform_(torch.empty(nh, H)))
        self.evolution = nn.ModuleDict({"gates": _tf_linear(2 * nh, 2 * nh, 1.0),
                                        "candidate": _tf_linear(2 * nh, nh)})
        width = self.num_dense_features + H + nh
        for key in ("userid", "device", "authorid", "bgm_song_id", "bgm_singer_id", "manual_tag_list"):
            width += self.embeddings[key].embedding_dim
        self.fcn = nn.ModuleList()
        self._tail = []
        for unit in hidden_units:
            lin = _tf_linear(width, unit)
            self.fcn.append(lin)
            if activation == 'dice':
                act, kind = Dice(unit), "dice"
            else:
                act, kind = nn.PReLU(), "prelu"
            self.fcn.append(act)
            bn = None
            if batch_norm:
                bn = nn.BatchNorm1d(unit)
                self.fcn.append(bn)
            if dropout_rate > 0:
                self.fcn.append(nn.Dropout(dropout_rate))
            self._tail.append(Layer(lin, act=kind, act_module=act, post_bn=bn))
            width = unit
        self.output_layer = _tf_linear(width, 1)

    def _load_vocabulary(self, vocab_dir, filename):
        return load_vocabulary(vocab_dir, filename)

    def interest_weights(self):
        """(Wg, bg, Wc, bc, A, Vg, vg, Vc, vc) as dien_interest takes them."""
        return (self.gru["gates"].weight, self.gru["gates"].bias, self.gru["candidate"].weight,
                self.gru["candidate"].bias, self.attention_project_matrix, self.evolution["gates"].weight,
                self.evolution["gates"].bias, self.evolution["candidate"].weight, self.evolution["candidate"].bias)

    def _plan(self, dense, category, sequence, target):
        """Row layout [dense | category | target | final interest state] and the gather segments
        (dien.py:179-191,237)."""
        dense_cols = [ops.as_f32(v, f"dense[{k!r}]") for k, v in dense.items()]
        B = dense_cols[0].shape[0]
        dev = dense_cols[0].device
        segs = [ops.dense_segment(v, 1, i) for i, v in enumerate(dense_cols)]
        col = len(dense_cols)
        for name, emb in self.embeddings.items():
            if name != "feedid" and name in category:
                segs.append(ops.table_segment(emb.weight, ops.as_index(category[name], f"category[{name!r}]"), col))
                col += emb.embedding_dim
        tgt = self.embeddings["feedid"]
        segs.append(ops.table_segment(tgt.weight, ops.as_index(target["feedid"], "target['feedid']"), col))
        q_col = col
        state_col = q_col + tgt.embedding_dim
        seq = ops.as_index(sequence[SEQ_KEY], f"sequence[{SEQ_KEY!r}]").contiguous()
        seq_len = ops.as_index(sequence[f"{SEQ_KEY}_length"], "sequence length").contiguous()
        return dict(B=B, dev=dev, segs=segs, q_col=q_col, state_col=state_col,
                    width=state_col + self.gru_output_units, H=tgt.embedding_dim, seq=seq, seq_len=seq_len)

    def forward(self, dense, category, sequence, target, return_attention=False):
        check_eval(self)
        tgt = target.get("feedid", None) if isinstance(target, dict) else None
        if isinstance(tgt, torch.Tensor) and tgt.shape[0] == 0:  # an empty batch: nothing to launch
            dev = ops.require_gpu(tgt, "target['feedid']").device
            return common.empty_rows(dev, 2)
        pl = self._plan(dense, category, sequence, target)
        B, dev, H, nh, width = pl["B"], pl["dev"], pl["H"], self.gru_output_units, pl["width"]
        if width != self._tail[0].linear.in_features:
            raise ValueError(f"rankops DIEN: the inputs make a row of {width} columns, the first fcn layer takes "
                             f"{self._tail[0].linear.in_features}")
        T = pl["seq"].shape[1]
        _check_envelope(H, nh, T)
        logit = torch.empty(B, 1, device=dev, dtype=torch.float32)
        prob = torch.empty(B, 1, device=dev, dtype=torch.float32)
        row = torch.empty(B, width, device=dev, dtype=torch.float32)
        att = torch.empty(B, T, device=dev, dtype=torch.float32) if return_attention else None
        ops.concat_gather(pl["segs"], B, row)
        try:
            ops.dien_interest(ops._lib.fptr(row, pl["q_col"]), width, self.embeddings["feedid"].weight, pl["seq"],
                              pl["seq_len"], T, H, nh, _cell(self.custom_gru_type), self.interest_weights(),
                              ops._lib.fptr(row, pl["state_col"]), width, att, B, dev)
        except ops._lib.RankOpsError as e:
            _convert(e, H, nh, T)
        run_tail(row, self._tail, self.output_layer, {}, logit, prob)
        return (prob, logit, att) if return_attention else (prob, logit)
