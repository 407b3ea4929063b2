"""CPU: the per-request ranking restatements (tests/ranking_ref.py) pinned against torch.topk and
sklearn, the conditions the fixed GPU test inputs must meet, and the argument checks of the new C
entry points (no device work is started on invalid input)."""
import ctypes

import numpy as np
import pytest
import torch

import ranking_ref as ref
import rankops
from rankops import _lib

sk = pytest.importorskip("sklearn.metrics")


def test_topk_restatement_equals_torch_topk_on_a_tie_free_rectangle():
    rng = np.random.default_rng(3)
    R, N, k = 7, 33, 10
    scores = rng.permutation(R * N).astype(np.float32) / 7.0  # distinct, finite
    values, indices, counts = ref.topk_ref(scores, ref.rows_of_segments(np.arange(R + 1) * N), k)
    want = torch.topk(torch.from_numpy(scores).view(R, N), k, dim=1)
    assert np.array_equal(values, want.values.numpy())
    assert np.array_equal(indices, want.indices.numpy() + (np.arange(R) * N)[:, None])
    assert np.array_equal(counts, np.full(R, k))


def test_topk_restatement_order_on_the_special_values():
    s = np.float32([0.0, np.nan, -np.inf, -0.0, np.inf, 1.0, np.nan, 1.0])
    values, indices, counts = ref.topk_ref(s, [np.arange(8)], 10)
    assert indices[0].tolist() == [4, 5, 7, 0, 3, 2, 1, 6, -1, -1] and counts[0] == 8
    assert np.isneginf(values[0, 8:]).all() and np.signbit(values[0, 4]) and not np.signbit(values[0, 3])


def test_topk_inputs_meet_their_conditions():
    scores, offsets = ref.topk_case()
    assert np.diff(offsets).tolist() == ref.TOPK_LENGTHS and ref.TOPK_KS == [1, 10, 64, 65, 200]
    route = rankops.ranking.topk_route  # by host-known arguments only: k 64 runs the segment kernel, 65 the sort path
    assert rankops.ranking.TOPK_SEGMENT_MAX_K == 64
    assert [route(int(offsets[-1]), len(ref.TOPK_LENGTHS), k) for k in ref.TOPK_KS] == ["segment"] * 3 + ["sort"] * 2
    assert route(512 * 7, 7, 10) == "segment" and route(512 * 7 + 1, 7, 10) == "sort" and route(0, 0, 1) == "segment"
    finite = scores[np.isfinite(scores)]
    assert len(np.unique(finite)) <= 8  # quantised: ties everywhere
    seg = lambda r: scores[offsets[r]:offsets[r + 1]]
    sp = seg(ref.SPECIAL_SEGMENT)
    assert np.isposinf(sp).any() and np.isneginf(sp).any()
    assert ((sp == 0) & np.signbit(sp)).any() and ((sp == 0) & ~np.signbit(sp)).any()
    assert np.isnan(seg(ref.NAN_SEGMENT)).sum() == 3 and np.isnan(scores).sum() == 3
    assert len(np.unique(seg(ref.TIED_SEGMENT))) == 1
    # in the special segment a -0.0 precedes a +0.0 among the best 64: the tie is decided by the row
    _, idx, _ = ref.topk_ref(scores, ref.rows_of_segments(offsets), 64)
    top = scores[idx[ref.SPECIAL_SEGMENT]]
    zeros = np.flatnonzero(top == 0)
    signs = np.signbit(top[zeros])
    assert (signs[1:] & ~signs[:-1]).any() and (~signs[1:] & signs[:-1]).any()  # each sign before the other
    assert (np.diff(idx[ref.SPECIAL_SEGMENT][zeros]) > 0).all()
    ps, req, R = ref.permuted_request_case()
    assert R == len(ref.TOPK_LENGTHS) and (req == -1).sum() == 1 and (req == R).sum() == 1
    assert sorted(np.bincount(req[(req >= 0) & (req < R)], minlength=R).tolist()) == sorted(ref.TOPK_LENGTHS)
    assert (np.diff(req) < 0).any()  # not grouped


def test_grouped_auc_restatement_matches_sklearn_per_group():
    for case in (ref.grouped_case(), ref.large_grouped_case(20_000, 300)):
        s, y, g = case
        got = ref.grouped_auc_ref(s, y, g)
        num = rows = 0.0
        for i, gid in enumerate(got["ids"]):
            m = g == gid
            assert (got["pos"][i], got["neg"][i]) == ((y[m] > 0.5).sum(), (y[m] <= 0.5).sum())
            if got["pos"][i] and got["neg"][i]:
                want = sk.roc_auc_score(y[m], s[m])
                assert abs(got["auc"][i] - want) < 1e-12
                assert abs(got["two_u"][i] / (2.0 * got["pos"][i] * got["neg"][i]) - want) < 1e-12
                num += m.sum() * want
                rows += m.sum()
            else:
                assert np.isnan(got["auc"][i])
        assert abs(got["gauc"] - num / rows) < 1e-12 and got["valid_rows"] == rows


def test_grouped_auc_inputs_meet_their_conditions():
    s, y, g = ref.grouped_case()
    got = ref.grouped_auc_ref(s, y, g)
    sizes = {ref.group_id(i): n for i, n in enumerate(ref.GROUP_SIZES)}
    assert ref.GROUP_SIZES == [0, 1, 2, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 1, 5, 300]
    assert got["ids"].tolist() == [i for i, n in sizes.items() if n]  # the empty group is absent
    assert (got["pos"] + got["neg"]).tolist() == [n for n in sizes.values() if n]
    assert got["valid_groups"] >= 8 and len(ref.GROUP_SIZES) - got["valid_groups"] >= 3
    assert len(np.unique(s)) <= 16 and (np.diff(g) < 0).any()
    auc = dict(zip(got["ids"].tolist(), got["auc"]))
    assert auc[ref.group_id(2)] == 0.0 and auc[ref.group_id(3)] == 0.5
    for i in (1, 4, 12, 13):
        assert np.isnan(auc[ref.group_id(i)])


def test_grouped_auc_restatement_ignores_out_of_range_groups_and_reports_nan():
    s, y, g = ref.grouped_case()
    base = ref.grouped_auc_ref(s, y, g)
    s2, y2 = np.r_[s, np.float32([0.9, 0.1])], np.r_[y, np.float32([0.0, 1.0])]
    got = ref.grouped_auc_ref(s2, y2, np.r_[g, [-5, 1 << 31]])
    assert got["gauc"] == base["gauc"] and np.array_equal(got["ids"], base["ids"])
    assert np.isnan(ref.grouped_auc_ref(s, np.ones_like(y), g)["gauc"])


def test_python_layer_names_and_cpu_refusal():
    for name in ("topk_segments", "topk_per_request", "grouped_auc", "RequestTopK", "GroupedAUC"):
        assert hasattr(rankops, name) and name in rankops.__all__
    assert callable(rankops.DIEN.rank) and callable(rankops.EvalAccumulator.grouped_auc)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rankops.topk_segments(torch.zeros(4), torch.tensor([0, 4]), 2)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rankops.topk_per_request(torch.zeros(4), torch.zeros(4, dtype=torch.int64), 1, 2)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rankops.grouped_auc(torch.zeros(4), torch.zeros(4), torch.zeros(4, dtype=torch.int64))


INVALID, UNSUPPORTED = 1, 4
P = 256  # a non-null stand-in: every call below must fail before it looks at a pointer's target


def test_new_entry_points_reject_bad_arguments_without_a_device():
    lib = _lib.load()
    nb = ctypes.c_int64()
    assert lib.rk_topk_by_request_workspace_size(1000, 11, ctypes.byref(nb)) == 0 and nb.value > 1000 * 24
    topk_ws = nb.value
    assert lib.rk_topk_by_request_workspace_size(-1, 11, ctypes.byref(nb)) == INVALID
    assert lib.rk_topk_by_request_workspace_size(1000, -1, ctypes.byref(nb)) == INVALID
    assert lib.rk_topk_by_request_workspace_size(1000, 11, None) == INVALID
    assert lib.rk_grouped_auc_workspace_size(1000, ctypes.byref(nb)) == 0 and nb.value > 1000 * 40
    auc_ws = nb.value
    assert lib.rk_grouped_auc_workspace_size(-1, ctypes.byref(nb)) == INVALID
    assert lib.rk_grouped_auc_workspace_size(1000, None) == INVALID

    seg = lambda **kw: lib.rk_topk_segments(*[kw.get(a, d) for a, d in (
        ("scores", P), ("n", 1000), ("offsets", P), ("R", 11), ("k", 10), ("values", P), ("indices", P),
        ("counts", P), ("stream", None))])
    for bad in ({"scores": None}, {"offsets": None}, {"values": None}, {"indices": None}, {"counts": None},
                {"k": 0}, {"k": 1025}, {"n": -1}, {"R": -1}):
        assert seg(**bad) == INVALID, bad
        assert "rk_topk_segments" in _lib.last_error()
    assert seg(k=65) == UNSUPPORTED  # a valid k outside the segment kernel's envelope

    for fn, second in ((lib.rk_topk_by_request, "request_index"), (lib.rk_topk_segments_sorted, "offsets")):
        def call(**kw):
            a = {"scores": P, second: P, "n": 1000, "R": 11, "k": 10, "values": P, "indices": P, "counts": P,
                 "workspace": P, "ws_bytes": topk_ws, "stream": None}
            a.update(kw)
            if second == "offsets":
                order = ("scores", "n", "offsets", "R", "k", "values", "indices", "counts", "workspace", "ws_bytes",
                         "stream")
            else:
                order = ("scores", "request_index", "n", "R", "k", "values", "indices", "counts", "workspace",
                         "ws_bytes", "stream")
            return fn(*[a[x] for x in order])
        for bad in ({"scores": None}, {second: None}, {"values": None}, {"indices": None}, {"counts": None},
                    {"workspace": None}, {"k": 0}, {"k": 1025}, {"n": -1}, {"R": -1}, {"ws_bytes": topk_ws - 1},
                    {"ws_bytes": 0}):
            assert call(**bad) == INVALID, (second, bad)

    def auc(**kw):
        a = {"scores": P, "labels": P, "groups": P, "n": 1000, "workspace": P, "ws_bytes": auc_ws, "summary": P,
             "group_ids": P, "two_u": P, "pos": P, "neg": P, "n_groups": P, "stream": None}
        a.update(kw)
        return lib.rk_grouped_auc(*a.values())
    for bad in ({"scores": None}, {"labels": None}, {"groups": None}, {"workspace": None}, {"summary": None},
                {"group_ids": None}, {"two_u": None}, {"pos": None}, {"neg": None}, {"n_groups": None}, {"n": -1},
                {"n": 0}, {"ws_bytes": auc_ws - 1}, {"ws_bytes": 0}):
        assert auc(**bad) == INVALID, bad
        assert "rk_grouped_auc" in _lib.last_error()
