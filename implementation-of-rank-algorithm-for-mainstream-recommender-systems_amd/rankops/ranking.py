"""Per-request ranking on the device: segmented top-K and grouped AUC (csrc/ranking.hip).

`DIEN.score` returns one flat [B, 1] column for the candidates of many requests.  A ranking stage
keeps the best k of each request; an evaluation reports the AUC per user and its impression-weighted
mean (GAUC, the metric of the DIN / DIEN papers).  Both are segmented operations over
(score, group), and a ragged batch has no padded [R, N] view for `torch.topk`.

    top = topk_segments(logit, offsets, k)                # candidates of request r: offsets[r]..offsets[r+1]
    top = topk_per_request(logit, request_index, R, k)    # request_index in any order
    top.values [R, k], top.indices [R, k] (rows of logit), top.counts [R]

Order: score descending, -0.0 == +0.0, NaN below every number, ties by the lower row; slots at or
past counts[r] = min(k, candidates of r) hold -inf / -1; values are the original bits of
scores[indices].  The two forms agree bit for bit.  1 <= k <= 1024.

    g = grouped_auc(prob, label, category["userid"])      # GroupedAUC(gauc, valid_groups, valid_rows)

device tensors, no synchronisation; `return_groups=True` adds the per-group integer table
(group id, 2U, P, N; AUC_g = 2U / (2 P N)) at the cost of one.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from . import _lib, ops

TOPK_MAX_K = 1024
# rk_topk_segments' envelope, and the longest mean segment (rows / requests, both known on the host)
# the segment kernel is the default for.  Measured (DESIGN.md §4b, B 32,768, k 10 and 64): the kernel
# takes 9 us at 128 rows per request and 30 us at 512 against the sort path's 49-51 us; at 2,048 it
# takes 73-112 us, a request being one wave's serial work, and the sort path is the default.
TOPK_SEGMENT_MAX_K = 64
TOPK_SEGMENT_MAX_MEAN_ROWS = 512


def topk_route(n: int, num_requests: int, k: int) -> str:
    """'segment' or 'sort' for topk_segments over n rows: host-known arguments only."""
    if k <= TOPK_SEGMENT_MAX_K and n <= TOPK_SEGMENT_MAX_MEAN_ROWS * max(num_requests, 1):
        return "segment"
    return "sort"


class RequestTopK(NamedTuple):
    values: torch.Tensor   # [R, k] float32
    indices: torch.Tensor  # [R, k] int64, rows of the flat score vector, -1 past counts
    counts: torch.Tensor   # [R] int64


class GroupedAUC(NamedTuple):
    gauc: torch.Tensor          # 0-d float64
    valid_groups: torch.Tensor  # 0-d int64: groups with both classes
    valid_rows: torch.Tensor    # 0-d int64: their rows


class GroupTable(NamedTuple):
    group_ids: torch.Tensor  # [G] int64, ascending
    two_u: torch.Tensor      # [G] int64, twice the Mann-Whitney U
    pos: torch.Tensor        # [G] int64
    neg: torch.Tensor        # [G] int64


def _scores(scores, what):
    ops.require_gpu(scores, f"{what}: scores")
    if scores.dim() == 2 and scores.shape[1] == 1:
        scores = scores.reshape(-1)
    if scores.dim() != 1:
        raise ValueError(f"rankops.{what}: scores must be [B] or [B, 1], got {tuple(scores.shape)}")
    return scores.detach().to(torch.float32).contiguous()


def _check_k(k, what):
    if not isinstance(k, int) or not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"rankops.{what}: k must be an integer in [1, {TOPK_MAX_K}], got {k!r}")


def _outputs(R, k, dev):
    return RequestTopK(torch.empty(R, k, dtype=torch.float32, device=dev),
                       torch.empty(R, k, dtype=torch.int64, device=dev),
                       torch.empty(R, dtype=torch.int64, device=dev))


def _topk_workspace(lib, n, R, dev):
    nb = ctypes.c_int64()
    _lib.check(lib.rk_topk_by_request_workspace_size(n, R, ctypes.byref(nb)), "rk_topk_by_request_workspace_size")
    return torch.empty(nb.value, dtype=torch.uint8, device=dev), nb.value


def topk_segments(scores: torch.Tensor, offsets: torch.Tensor, k: int, method: str = None) -> RequestTopK:
    """The best k candidates of each request, request r owning the contiguous rows
    offsets[r] .. offsets[r+1] of scores (offsets [R+1], non-decreasing).  `method` None picks by
    topk_route(rows, R, k): "segment" (one wave per request, one launch) for k <= 64 and at most 512
    rows per request on average, "sort" otherwise; either may be forced, "segment" only for k <= 64."""
    lib = _lib.load()
    s = _scores(scores, "topk_segments")
    _check_k(k, "topk_segments")
    off = ops.as_index(offsets, "topk_segments: offsets")
    if off.dim() != 1 or off.shape[0] < 1 or off.device != s.device:
        raise ValueError(f"rankops.topk_segments: offsets must be [R + 1] on {s.device}, got {tuple(off.shape)}")
    off = off.contiguous()
    R, n = off.shape[0] - 1, s.numel()
    if method is None:
        method = topk_route(n, R, k)
    if method not in ("segment", "sort"):
        raise ValueError(f"rankops.topk_segments: method must be 'segment' or 'sort', got {method!r}")
    _lib.ensure_device(s.device)
    out = _outputs(R, k, s.device)
    if method == "segment":
        _lib.check(lib.rk_topk_segments(s.data_ptr(), n, off.data_ptr(), R, k, out.values.data_ptr(),
                                        out.indices.data_ptr(), out.counts.data_ptr(), _lib.stream_of(s)),
                   "rk_topk_segments")
    else:
        ws, nb = _topk_workspace(lib, n, R, s.device)
        _lib.check(lib.rk_topk_segments_sorted(s.data_ptr(), n, off.data_ptr(), R, k, out.values.data_ptr(),
                                               out.indices.data_ptr(), out.counts.data_ptr(), ws.data_ptr(), nb,
                                               _lib.stream_of(s)), "rk_topk_segments_sorted")
    return out


def topk_per_request(scores: torch.Tensor, request_index: torch.Tensor, num_requests: int, k: int) -> RequestTopK:
    """The best k candidates of each of `num_requests` requests, row b belonging to request
    request_index[b] (any order).  A request_index outside [0, num_requests) is left out and raises
    RK_FLAG_INDEX_OOB (rankops.error_flags), as DIEN.score does."""
    lib = _lib.load()
    s = _scores(scores, "topk_per_request")
    _check_k(k, "topk_per_request")
    req = ops.as_index(request_index, "topk_per_request: request_index")
    if req.dim() != 1 or req.shape[0] != s.numel() or req.device != s.device:
        raise ValueError(f"rankops.topk_per_request: request_index must be [{s.numel()}] on {s.device}, one request "
                         f"per score, got {tuple(req.shape)}")
    if not isinstance(num_requests, int) or num_requests < 0:
        raise ValueError(f"rankops.topk_per_request: num_requests must be a non-negative integer, got {num_requests!r}")
    req = req.contiguous()
    R, n = num_requests, s.numel()
    _lib.ensure_device(s.device)
    out = _outputs(R, k, s.device)
    ws, nb = _topk_workspace(lib, n, R, s.device)
    _lib.check(lib.rk_topk_by_request(s.data_ptr(), req.data_ptr(), n, R, k, out.values.data_ptr(),
                                      out.indices.data_ptr(), out.counts.data_ptr(), ws.data_ptr(), nb,
                                      _lib.stream_of(s)), "rk_topk_by_request")
    return out


def grouped_auc(scores: torch.Tensor, labels: torch.Tensor, groups: torch.Tensor, return_groups: bool = False):
    """AUC per group (exact: Mann-Whitney U with ties credited 1/2, from integer counts) and GAUC,
    the mean of the per-group AUCs weighted by the group's row count over the groups that hold both
    classes.  Returns GroupedAUC(gauc, valid_groups, valid_rows) as 0-d device tensors without a
    synchronisation; gauc is NaN when no group is valid or a valid group holds a NaN score.  Group
    ids lie in [0, 2^31); others are left out and raise RK_FLAG_INDEX_OOB.  With return_groups=True:
    (GroupedAUC, GroupTable) — one row per group present, ascending id — which synchronises once."""
    lib = _lib.load()
    s = _scores(scores, "grouped_auc")
    ops.require_gpu(labels, "grouped_auc: labels")
    y = labels.detach().reshape(-1).to(torch.float32).contiguous()
    g = ops.as_index(groups, "grouped_auc: groups").detach().reshape(-1).contiguous()
    n = s.numel()
    if y.numel() != n or g.numel() != n or y.device != s.device or g.device != s.device:
        raise ValueError(f"rankops.grouped_auc: {n} scores, {y.numel()} labels, {g.numel()} groups must match on "
                         f"one device")
    if n == 0:
        raise ValueError("rankops.grouped_auc: no rows")
    _lib.ensure_device(s.device)
    nb = ctypes.c_int64()
    _lib.check(lib.rk_grouped_auc_workspace_size(n, ctypes.byref(nb)), "rk_grouped_auc_workspace_size")
    ws = torch.empty(nb.value, dtype=torch.uint8, device=s.device)
    summary = torch.empty(3, dtype=torch.float64, device=s.device)  # [double | int64 | int64]
    table = torch.empty(4, n, dtype=torch.int64, device=s.device)
    n_groups = torch.empty((), dtype=torch.int64, device=s.device)
    _lib.check(lib.rk_grouped_auc(s.data_ptr(), y.data_ptr(), g.data_ptr(), n, ws.data_ptr(), nb.value,
                                  summary.data_ptr(), table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(),
                                  table[3].data_ptr(), n_groups.data_ptr(), _lib.stream_of(s)), "rk_grouped_auc")
    counts = summary.view(torch.int64)
    res = GroupedAUC(summary[0], counts[1], counts[2])
    if not return_groups:
        return res
    G = int(n_groups)
    return res, GroupTable(*(table[i, :G] for i in range(4)))
