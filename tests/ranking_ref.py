"""numpy restatements of the per-request ranking contract (include/rankops.h, csrc/ranking.hip) and
the fixed inputs the CPU and GPU tests share.

Top-K: within a request, score descending, -0.0 == +0.0, NaN below every number (-inf included),
ties by the lower row; values [R, k] are scores[indices], indices [R, k] rows of the flat score
vector, counts [R] = min(k, n_r); slots at or past counts[r] hold -inf / -1.
Grouped AUC: per group the exact AUC (oracle.metrics.roc_auc) and the integers 2U, P, N; GAUC is the
mean of the AUCs of the groups with both classes weighted by the group's row count, in float64.
"""
import numpy as np

from oracle import metrics as oracle_metrics

# ---------------------------------------------------------------- top-K


def topk_order(scores, rows):
    """`rows` (row numbers into scores) in the contract's order, best first."""
    rows = np.asarray(rows, np.int64)
    s = np.asarray(scores, np.float32)[rows].astype(np.float64)
    nan = np.isnan(s)
    neg = np.where(nan, 0.0, -s) + 0.0  # descending score; -0.0 and +0.0 compare equal
    return rows[np.lexsort((rows, neg, nan))]  # last key first: numbers before NaN, score, row


def topk_ref(scores, rows_of_request, k):
    """rows_of_request: one array of row numbers per request.  Returns (values float32 [R, k],
    indices int64 [R, k], counts int64 [R])."""
    scores = np.asarray(scores, np.float32).reshape(-1)
    R = len(rows_of_request)
    values = np.full((R, k), -np.inf, np.float32)
    indices = np.full((R, k), -1, np.int64)
    counts = np.zeros(R, np.int64)
    for r, rows in enumerate(rows_of_request):
        best = topk_order(scores, rows)[:k]
        counts[r] = len(best)
        indices[r, :len(best)] = best
        values[r, :len(best)] = scores[best]
    return values, indices, counts


def rows_of_segments(offsets):
    offsets = np.asarray(offsets, np.int64)
    return [np.arange(offsets[r], offsets[r + 1], dtype=np.int64) for r in range(len(offsets) - 1)]


def rows_of_request_index(request_index, R):
    request_index = np.asarray(request_index, np.int64)
    return [np.flatnonzero(request_index == r).astype(np.int64) for r in range(R)]


TOPK_LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 1000, 0]
TOPK_KS = [1, 10, 64, 65, 200]
SPECIAL_SEGMENT, TIED_SEGMENT, NAN_SEGMENT = 5, 6, 7  # lengths 65, 127, 128


def topk_case(seed=20241):
    """(scores float32 [B], offsets int64 [R + 1]) over TOPK_LENGTHS: scores on 8 levels (one of them
    0.0), segment 5 with +inf, -inf, -0.0, +0.0, segment 6 all tied, segment 7 with three NaNs."""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(TOPK_LENGTHS)]).astype(np.int64)
    scores = ((rng.integers(0, 8, offsets[-1]) - 4) / 8.0).astype(np.float32)
    o = offsets[SPECIAL_SEGMENT]
    scores[o + 3:o + 7] = [-0.0, 0.0, -0.0, 0.0]
    scores[o + 20], scores[o + 41] = np.inf, -np.inf
    scores[o + 50], scores[o + 64] = -0.0, np.inf
    scores[offsets[TIED_SEGMENT]:offsets[TIED_SEGMENT + 1]] = 0.25
    o = offsets[NAN_SEGMENT]
    scores[[o, o + 70, o + 127]] = np.nan
    scores[o + 5] = -np.inf  # NaN ranks below it
    return scores, offsets


def permuted_request_case(seed=20242):
    """topk_case's candidates under a seeded permutation, plus two rows whose request_index is -1 and
    R.  Returns (scores [B + 2], request_index [B + 2], R)."""
    scores, offsets = topk_case()
    R = len(offsets) - 1
    req = np.repeat(np.arange(R, dtype=np.int64), np.diff(offsets))
    scores = np.concatenate([scores, np.float32([9.0, 9.0])])  # would win any request they joined
    req = np.concatenate([req, np.int64([-1, R])])
    perm = np.random.default_rng(seed).permutation(len(scores))
    return scores[perm], req[perm], R


# ---------------------------------------------------------------- grouped AUC

GROUP_ID_LIMIT = 1 << 31


def two_u_pairs(scores, labels):
    """2U, P, N of one group by counting over every (positive, negative) pair: 2 for a positive above
    a negative, 1 for a tie."""
    s = np.asarray(scores, np.float32).astype(np.float64)
    pos = np.asarray(labels, np.float32) > 0.5
    sp, sn = s[pos][:, None], s[~pos][None, :]
    return int(2 * np.sum(sp > sn) + np.sum(sp == sn)), int(pos.sum()), int((~pos).sum())


def grouped_auc_ref(scores, labels, groups):
    """Returns a dict: ids, two_u, pos, neg (int64 arrays, ascending group id, groups in
    [0, 2^31) only), auc (float64 per group, NaN where a class is missing), gauc, valid_groups,
    valid_rows."""
    scores = np.asarray(scores, np.float32).reshape(-1)
    labels = np.asarray(labels, np.float32).reshape(-1)
    groups = np.asarray(groups, np.int64).reshape(-1)
    keep = (groups >= 0) & (groups < GROUP_ID_LIMIT)
    order = np.argsort(groups[keep], kind="stable")
    s, y, g = scores[keep][order], labels[keep][order], groups[keep][order]
    ids, starts = np.unique(g, return_index=True)
    ends = np.r_[starts[1:], len(g)]
    two_u, pos, neg, auc = [], [], [], []
    num, rows, valid = 0.0, 0, 0
    for a, b in zip(starts, ends):
        u, p, q = two_u_pairs(s[a:b], y[a:b])
        two_u.append(u), pos.append(p), neg.append(q)
        auc.append(oracle_metrics.roc_auc(s[a:b], y[a:b]) if p and q else float("nan"))
        if p and q:
            valid += 1
            rows += b - a
            num += float(b - a) * auc[-1]
    return {"ids": ids.astype(np.int64), "two_u": np.array(two_u, np.int64), "pos": np.array(pos, np.int64),
            "neg": np.array(neg, np.int64), "auc": np.array(auc, np.float64),
            "gauc": num / rows if valid else float("nan"), "valid_groups": valid, "valid_rows": int(rows)}


GROUP_SIZES = [0, 1, 2, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 1, 5, 300]


def group_id(i):
    return 7 * i + 2  # ids with gaps, not the positions


def grouped_case(seed=20243):
    """(scores, labels, groups) over GROUP_SIZES, rows interleaved by a seeded permutation: scores on a
    16-level grid, labels at rate 0.3, and the small groups set by hand — groups 1 and 12 (one row)
    and 4 (three positives), 13 (five negatives) single-class; group 2 one positive below one
    negative (AUC 0); group 3 one tie (AUC 1/2)."""
    rng = np.random.default_rng(seed)
    n = sum(GROUP_SIZES)
    groups = np.repeat([group_id(i) for i in range(len(GROUP_SIZES))], GROUP_SIZES).astype(np.int64)
    scores = (rng.integers(0, 16, n) / 16.0).astype(np.float32)
    labels = (rng.random(n) < 0.3).astype(np.float32)
    start = np.concatenate([[0], np.cumsum(GROUP_SIZES)])
    labels[start[1]], labels[start[12]] = 1.0, 0.0
    scores[start[2]:start[3]], labels[start[2]:start[3]] = [0.25, 0.75], [1.0, 0.0]
    scores[start[3]:start[4]], labels[start[3]:start[4]] = [0.5, 0.5], [0.0, 1.0]
    labels[start[4]:start[5]] = 1.0
    labels[start[13]:start[14]] = 0.0
    perm = rng.permutation(n)
    return scores[perm], labels[perm], groups[perm]


def large_grouped_case(n=200_000, n_groups=5_000, seed=20244):
    rng = np.random.default_rng(seed)
    groups = rng.integers(0, n_groups, n).astype(np.int64) * 3
    scores = (rng.integers(0, 64, n) / 64.0).astype(np.float32)
    labels = (rng.random(n) < 0.3).astype(np.float32)
    return scores, labels, groups
