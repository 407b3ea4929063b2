"""GPU: per-request ranking (rankops.ranking over csrc/ranking.hip) against the numpy restatements
of tests/ranking_ref.py — segmented top-K in both forms, grouped AUC / GAUC, EvalAccumulator with
groups, DIEN.rank, and both under graph capture.  The integers (indices, counts, the per-group
table) are exact; GAUC is within 1e-12 of the float64 restatement (the tolerance test_gpu_metrics.py
uses for the same integer scheme: above the (G + 2) 2^-53 a reordered double sum can differ by) and
bit-equal under a permutation of the rows."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
import ranking_ref as ref
import rankops
from test_gpu_dien_requests import model_and_requests

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    """Floats as their int32 bits: NaN equals itself, -0.0 differs from +0.0."""
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def check_topk(got, scores, want, k):
    values, indices, counts = (t.cpu().numpy() for t in got)
    w_values, w_indices, w_counts = want
    R = len(w_counts)
    assert values.shape == (R, k) and indices.shape == (R, k) and counts.shape == (R,)
    assert values.dtype == np.float32 and indices.dtype == np.int64 and counts.dtype == np.int64
    assert np.array_equal(counts, w_counts)
    assert np.array_equal(indices, w_indices)
    live = np.arange(k)[None, :] < counts[:, None]
    assert np.array_equal(values[live].view(np.int32), scores[indices[live]].view(np.int32))  # the original bits
    assert np.isneginf(values[~live]).all() and (indices[~live] == -1).all()
    assert np.array_equal(values.view(np.int32), w_values.view(np.int32))


@functools.lru_cache(maxsize=None)
def segment_want(k):
    scores, offsets = ref.topk_case()
    return ref.topk_ref(scores, ref.rows_of_segments(offsets), k)


@pytest.mark.parametrize("k", ref.TOPK_KS)
def test_topk_segments_equals_the_restatement(k):
    scores, offsets = ref.topk_case()
    got = rankops.topk_segments(cuda(scores), cuda(offsets), k)
    assert isinstance(got, rankops.RequestTopK)
    check_topk(got, scores, segment_want(k), k)
    col = rankops.topk_segments(cuda(scores).view(-1, 1), cuda(offsets), k)  # [B, 1] as DIEN.score returns it
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, col))
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("k", [1, 10, 64])
def test_topk_segments_kernel_and_sort_path_agree_bit_for_bit(k):
    scores, offsets = ref.topk_case()
    a = rankops.topk_segments(cuda(scores), cuda(offsets), k, method="segment")
    b = rankops.topk_segments(cuda(scores), cuda(offsets), k, method="sort")
    req = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    c = rankops.topk_per_request(cuda(scores), cuda(req), len(offsets) - 1, k)
    for x, y, z in zip(a, b, c):
        assert torch.equal(bits(x), bits(y)) and torch.equal(bits(y), bits(z))
    check_topk(b, scores, segment_want(k), k)
    assert rankops.error_flags() == 0


def test_topk_segments_offsets_inside_a_longer_score_vector_and_out_of_range():
    scores, offsets = ref.topk_case()
    padded = np.concatenate([np.float32([7.0] * 5), scores, np.float32([8.0] * 3)])  # rows no segment covers
    for method in ("segment", "sort"):
        got = rankops.topk_segments(cuda(padded), cuda(offsets + 5), 10, method=method)
        check_topk(got, padded, ref.topk_ref(padded, ref.rows_of_segments(offsets + 5), 10), 10)
    assert rankops.error_flags() == 0
    # one long segment: past 512 rows per request the default is the sort path
    whole = np.int64([0, len(scores)])
    assert rankops.ranking.topk_route(len(scores), 1, 10) == "sort"
    for method in (None, "segment"):
        got = rankops.topk_segments(cuda(scores), cuda(whole), 10, method=method)
        check_topk(got, scores, ref.topk_ref(scores, ref.rows_of_segments(whole), 10), 10)
    # an offset past the scores is clamped, never read, and flagged
    bad = np.int64([0, 3, len(scores) + 100])
    for method in ("segment", "sort"):
        got = rankops.topk_segments(cuda(scores), cuda(bad), 4, method=method)
        check_topk(got, scores, ref.topk_ref(scores, ref.rows_of_segments(np.int64([0, 3, len(scores)])), 4), 4)
        assert rankops.error_flags() == 1


@pytest.mark.parametrize("k", ref.TOPK_KS)
def test_topk_per_request_any_order_and_out_of_range_requests(k):
    scores, req, R = ref.permuted_request_case()
    got = rankops.topk_per_request(cuda(scores), cuda(req), R, k)
    want = ref.topk_ref(scores, ref.rows_of_request_index(req, R), k)
    check_topk(got, scores, want, k)
    left_out = np.flatnonzero((req < 0) | (req >= R))
    assert len(left_out) == 2 and not np.isin(got.indices.cpu().numpy(), left_out).any()
    assert rankops.error_flags() == 1  # RK_FLAG_INDEX_OOB
    assert rankops.error_flags() == 0


def test_topk_per_request_one_request_and_no_candidates():
    scores, _ = ref.topk_case()
    one = np.zeros(len(scores), np.int64)
    for k in (10, 200):
        got = rankops.topk_per_request(cuda(scores), cuda(one), 1, k)
        check_topk(got, scores, ref.topk_ref(scores, [np.arange(len(scores))], k), k)
    for k in (3, 100):  # B = 0: every slot is padding
        got = rankops.topk_per_request(torch.empty(0, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda"),
                                       4, k)
        check_topk(got, np.empty(0, np.float32), ref.topk_ref(np.empty(0, np.float32), [np.empty(0, np.int64)] * 4, k),
                   k)
        got = rankops.topk_segments(torch.empty(0, device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda"), k)
        assert (got.counts == 0).all() and (got.indices == -1).all() and torch.isneginf(got.values).all()
    assert rankops.error_flags() == 0
    with pytest.raises(ValueError):
        rankops.topk_per_request(cuda(scores), cuda(one), 1, 0)
    with pytest.raises(ValueError):
        rankops.topk_segments(cuda(scores), cuda(np.int64([0, 4])), 1025)


# ---------------------------------------------------------------- grouped AUC

def check_grouped(got, table, want):
    assert isinstance(got, rankops.GroupedAUC)
    assert got.gauc.dtype == torch.float64 and got.valid_groups.dtype == torch.int64
    ids, two_u, pos, neg = (t.cpu().numpy() for t in table)
    assert np.array_equal(ids, want["ids"])
    assert np.array_equal(pos, want["pos"]) and np.array_equal(neg, want["neg"])
    assert np.array_equal(two_u, want["two_u"])
    assert int(got.valid_groups) == want["valid_groups"] and int(got.valid_rows) == want["valid_rows"]
    print(f"gauc {float(got.gauc)!r} restatement {want['gauc']!r} diff {abs(float(got.gauc) - want['gauc']):.3e}")
    assert abs(float(got.gauc) - want["gauc"]) < 1e-12


@functools.lru_cache(maxsize=None)
def grouped_want():
    return ref.grouped_auc_ref(*ref.grouped_case())


def test_grouped_auc_table_is_exact_and_gauc_matches():
    s, y, g = ref.grouped_case()
    got, table = rankops.grouped_auc(cuda(s), cuda(y), cuda(g), return_groups=True)
    check_grouped(got, table, grouped_want())
    alone = rankops.grouped_auc(cuda(s).view(-1, 1), cuda(y).view(-1, 1), cuda(g))
    assert torch.equal(alone.gauc, got.gauc) and alone.gauc.dim() == 0
    assert rankops.error_flags() == 0


def test_grouped_auc_is_bit_equal_under_a_permutation_of_the_rows():
    s, y, g = ref.grouped_case()
    base = rankops.grouped_auc(cuda(s), cuda(y), cuda(g))
    for seed in (1, 2):
        p = np.random.default_rng(seed).permutation(len(s))
        got, table = rankops.grouped_auc(cuda(s[p]), cuda(y[p]), cuda(g[p]), return_groups=True)
        assert torch.equal(got.gauc.view(torch.int64), base.gauc.view(torch.int64))
        check_grouped(got, table, grouped_want())


def test_grouped_auc_nan_score_single_class_and_bad_group_ids():
    s, y, g = ref.grouped_case()
    want = grouped_want()
    big = int(want["ids"][np.argmax(want["pos"] + want["neg"])])
    s_nan = s.copy()
    s_nan[np.flatnonzero(g == big)[3]] = np.nan
    assert np.isnan(ref.grouped_auc_ref(s_nan, y, g)["gauc"])
    got = rankops.grouped_auc(cuda(s_nan), cuda(y), cuda(g))
    assert np.isnan(float(got.gauc)) and int(got.valid_groups) == want["valid_groups"]
    got = rankops.grouped_auc(cuda(s), cuda(np.ones_like(y)), cuda(g))
    assert np.isnan(float(got.gauc)) and int(got.valid_groups) == 0 and int(got.valid_rows) == 0
    assert rankops.error_flags() == 0
    # ids outside [0, 2^31) are left out (these two rows alone would form a valid group) and flagged
    s2, y2 = np.r_[s, np.float32([0.9, 0.1, 0.5])], np.r_[y, np.float32([0.0, 1.0, 1.0])]
    g2 = np.r_[g, np.int64([-5, -5, 1 << 31])]
    got, table = rankops.grouped_auc(cuda(s2), cuda(y2), cuda(g2), return_groups=True)
    check_grouped(got, table, want)
    assert rankops.error_flags() == 1
    top = np.r_[g, np.int64([(1 << 31) - 1] * 2)]  # the largest valid id is a group like any other
    got, table = rankops.grouped_auc(cuda(s2[:-1]), cuda(y2[:-1]), cuda(top), return_groups=True)
    check_grouped(got, table, ref.grouped_auc_ref(s2[:-1], y2[:-1], top))
    assert rankops.error_flags() == 0


def test_grouped_auc_large_multi_block():
    s, y, g = ref.large_grouped_case()
    got, table = rankops.grouped_auc(cuda(s), cuda(y), cuda(g), return_groups=True)
    check_grouped(got, table, ref.grouped_auc_ref(s, y, g))
    assert rankops.error_flags() == 0


def test_eval_accumulator_grouped_auc_over_ragged_batches():
    rng = np.random.default_rng(5)
    with_groups, plain = rankops.EvalAccumulator("cuda", loss="bce"), rankops.EvalAccumulator("cuda", loss="bce")
    ps, ys, gs = [], [], []
    for B in (4096, 1000, 7):
        p = (rng.integers(1, 32, B) / 32.0).astype(np.float32)
        y = (rng.random(B) < 0.3).astype(np.float32)
        g = rng.integers(0, 200, B).astype(np.int64)
        with_groups.add(cuda(p), cuda(y), groups=cuda(g))
        plain.add(cuda(p), cuda(y))
        ps.append(p), ys.append(y), gs.append(g)
    got, table = with_groups.grouped_auc(return_groups=True)
    check_grouped(got, table, ref.grouped_auc_ref(np.concatenate(ps), np.concatenate(ys), np.concatenate(gs)))
    with_r, plain_r = with_groups.result(), plain.result()  # the loss sum is an atomic double: last bits may differ
    assert len(with_r) == 3 and with_r[1:] == plain_r[1:] and abs(with_r[0] - plain_r[0]) < 1e-12
    with pytest.raises(ValueError, match="without groups"):
        plain.grouped_auc()
    with_groups.add(cuda(ps[0]), cuda(ys[0]))
    with pytest.raises(ValueError, match="without groups"):
        with_groups.grouped_auc()
    with pytest.raises(TypeError):
        with_groups.add(cuda(ps[0]), cuda(ys[0]), None, None, cuda(gs[0]))  # keyword only


def test_dien_rank_is_score_then_topk_on_the_logit():
    R, B, k = 5, 37, 4
    m, history, inp, req = model_and_requests("AUGRU", R=R, B=B, T=20)
    req[req == 3] = 1  # request 3 has no candidate
    m = m.cuda()
    d_inp, d_hist, d_req = H.to_device(inp, "cuda"), H.to_device(history, "cuda"), req.cuda()
    interests = m.extract_interests(d_hist)
    prob, logit = m.score(d_inp["dense"], d_inp["category"], d_inp["target"], interests, d_req)
    top, r_prob, r_logit = m.rank(d_inp["dense"], d_inp["category"], d_inp["target"], interests, d_req, k)
    assert torch.equal(r_prob, prob) and torch.equal(r_logit, logit) and r_logit.shape == (B, 1)
    scores = logit.cpu().numpy().reshape(-1)
    check_topk(top, scores, ref.topk_ref(scores, ref.rows_of_request_index(req.numpy(), R), k), k)
    assert int(top.counts[3]) == 0
    assert rankops.error_flags() == 0
    with pytest.raises(NotImplementedError, match="eval"):
        m.train().rank(d_inp["dense"], d_inp["category"], d_inp["target"], interests, d_req, k)


def test_topk_and_grouped_auc_replay_in_one_graph():
    scores, offsets = ref.topk_case()
    s, y, g = ref.grouped_case()
    k = 10
    d_scores, d_off = cuda(scores), cuda(offsets)
    d_s, d_y, d_g = cuda(s), cuda(y), cuda(g)
    rankops.topk_segments(d_scores, d_off, k)  # the first call initialises the device state
    rankops.grouped_auc(d_s, d_y, d_g)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        top = rankops.topk_segments(d_scores, d_off, k)
        auc = rankops.grouped_auc(d_s, d_y, d_g)
    # new inputs, written in place: other scores in other segments, other rows in the groups
    rng = np.random.default_rng(9)
    scores2 = rng.permutation(scores)
    offsets2 = np.concatenate([[0], np.cumsum(ref.TOPK_LENGTHS[::-1])]).astype(np.int64)
    p = rng.permutation(len(s))
    s2, y2, g2 = (rng.integers(0, 16, len(s)) / 16.0).astype(np.float32), y[p], g
    d_scores.copy_(cuda(scores2)), d_off.copy_(cuda(offsets2))
    d_s.copy_(cuda(s2)), d_y.copy_(cuda(y2)), d_g.copy_(cuda(g2))
    graph.replay()
    torch.cuda.synchronize()
    check_topk(top, scores2, ref.topk_ref(scores2, ref.rows_of_segments(offsets2), k), k)
    want = ref.grouped_auc_ref(s2, y2, g2)
    assert abs(float(auc.gauc) - want["gauc"]) < 1e-12
    assert int(auc.valid_groups) == want["valid_groups"] and int(auc.valid_rows) == want["valid_rows"]
    assert rankops.error_flags() == 0
