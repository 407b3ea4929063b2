"""Float64 restatement of rk_sparse_adam_step (torch.optim.SparseAdam / TF LazyAdam), the case
table of tests/test_gpu_sparse_adam.py, and the tolerances of the GPU tests.

The step, for every distinct row r of a table's sparse gradient, with g the sum of the row's entries:
    m[r] += (1 - beta1) (g - m[r])
    v[r] += (1 - beta2) (g^2 - v[r])
    p[r] -= lr sqrt(1 - beta2^t) / (1 - beta1^t) * m[r] / (sqrt(v[r]) + eps)
Rows that are not in the gradient stay as they are; an id outside [0, rows) contributes nothing.

Input condition.  The update divides by sqrt(v) ~ |g|, so it is ill-conditioned where a run's sum
is near zero.  Values are s[row, col] * u with u uniform in [0.5, 1.5] and one random sign per
(row, column), kept over the steps: every run's |sum| is then >= 0.5 in every column, which
make_case asserts, a row's first moment never cancels from one step to the next, and no case has
to be left out.

Tolerances.  REL[k] bounds the error of tensor k (param, exp_avg, exp_avg_sq) after each step of a
case: for param max|got - want| / max|want| over the tensor (Adam moves every element by about lr
whatever its size, so the error is uniform over the rows), for the two moments the largest
per-row max|got - want| / max|want| (a padded history's hot row holds moments a thousand times
those of the other rows, which a tensor-wide scale would hide; under the input condition every
row's moments are bounded away from zero).  REL is MARGIN = 50 x DRIFT, the largest such error of
a float32 run of this restatement against the float64 one over the case table (the project's
margin, tests/test_train_ops_ref.py), recorded to three digits.  tests/test_sparse_adam_host.py
measures the drift again and holds DRIFT to it."""
import zlib

import torch

LR, BETAS, EPS, STEPS = 1e-2, (0.9, 0.999), 1e-8, 3

# the measured float32 drift (test_sparse_adam_host.py::test_float32_drift_sets_the_gpu_tolerances),
# the moments' from the 8192-entry runs' float32 sums
DRIFT = {"param": 1.12e-7, "exp_avg": 2.97e-6, "exp_avg_sq": 5.85e-6}
MARGIN = 50.0
REL = {k: MARGIN * v for k, v in DRIFT.items()}
PER_ROW = {"param": False, "exp_avg": True, "exp_avg_sq": True}


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def table(rows, dim, nnz, mode="random", idx_stride=1, value_pad=0, coalesced=False):
    return dict(rows=rows, dim=dim, nnz=nnz, mode=mode, idx_stride=idx_stride, value_pad=value_pad,
                coalesced=coalesced)


CASES = {}
for _d in (1, 6, 32):
    for _r in (1, 7, 1000):
        for _n in (1, 63, 64, 65, 4097):
            CASES[f"d{_d}_r{_r}_n{_n}"] = [table(_r, _d, _n)]
CASES["one_row_n8192"] = [table(1000, 32, 8192, mode="one_row")]
CASES["one_row_n8192_d6"] = [table(7, 6, 8192, mode="one_row")]
CASES["distinct"] = [table(1000, 6, 1000, mode="distinct")]
CASES["idx_stride2"] = [table(1000, 6, 300, idx_stride=2)]
CASES["value_stride"] = [table(1000, 6, 300, value_pad=5), table(7, 1, 65, value_pad=3)]
CASES["three_tables"] = [table(1000, 1, 300), table(7, 6, 4097), table(1000, 32, 65)]
CASES["coalesced"] = [table(1000, 32, 300, mode="distinct", coalesced=True)]
CASES["coalesced_and_sorted"] = [table(1000, 6, 65, mode="distinct", coalesced=True), table(1000, 6, 4097),
                                 table(7, 1, 7, mode="distinct", coalesced=True)]
# a padded history list: most of B x T positions on the padding row, the rest spread out
CASES["padded_history"] = [table(1000, 32, 4096, mode="padded")]


def make_case(name):
    """Per table of CASES[name]: dict(spec, p0 float64 [rows, dim], steps: STEPS x (idx int64 [nnz],
    values float64 [nnz, dim]))."""
    out = []
    for k, spec in enumerate(CASES[name]):
        rows, dim, nnz = spec["rows"], spec["dim"], spec["nnz"]
        g = gen("sparse_adam", name, k)
        p0 = torch.randn(rows, dim, generator=g, dtype=torch.float64)
        sign = torch.randint(0, 2, (rows, dim), generator=g).double() * 2 - 1
        steps = []
        for _ in range(STEPS):
            if spec["mode"] == "one_row":
                idx = torch.full((nnz,), min(5, rows - 1), dtype=torch.int64)
            elif spec["mode"] == "distinct":
                idx = torch.randperm(rows, generator=g)[:nnz]
                if spec["coalesced"]:
                    idx = idx.sort().values
            elif spec["mode"] == "padded":
                idx = torch.randint(0, rows, (nnz,), generator=g)
                idx[torch.rand(nnz, generator=g) < 0.8] = 0
            else:
                idx = torch.randint(0, rows, (nnz,), generator=g)
            u = torch.rand(nnz, dim, generator=g, dtype=torch.float64) + 0.5
            vals = sign[idx] * u
            sums = torch.zeros(rows, dim, dtype=torch.float64).index_add_(0, idx, vals)
            assert bool((sums[idx.unique()].abs() >= 0.5).all()), "input condition: every run's |sum| >= 0.5"
            steps.append((idx, vals))
        out.append(dict(spec=spec, p0=p0, steps=steps))
    return out


def sparse_adam_step(p, m, v, idx, vals, t, lr=LR, betas=BETAS, eps=EPS):
    """One step in place on p, m, v [rows, dim] (any float dtype) from the gradient entries
    (idx [nnz], vals [nnz, dim]); t is the 1-based step count.  Ids outside [0, rows) are dropped."""
    ok = (idx >= 0) & (idx < p.shape[0])
    idx, vals = idx[ok], vals[ok].to(p.dtype)
    if idx.numel() == 0:
        return
    rows, inv = torch.unique(idx, return_inverse=True)
    g = torch.zeros(rows.numel(), p.shape[1], dtype=p.dtype).index_add_(0, inv, vals)
    beta1, beta2 = betas
    m_r = m[rows] + (1 - beta1) * (g - m[rows])
    v_r = v[rows] + (1 - beta2) * (g * g - v[rows])
    step_size = lr * (1 - beta2 ** t) ** 0.5 / (1 - beta1 ** t)
    m[rows], v[rows] = m_r, v_r
    p[rows] = p[rows] - step_size * (m_r / (v_r.sqrt() + eps))


def run_case(case, dtype=torch.float64):
    """The case's STEPS steps from zero moments; returns per step, per table (p, m, v) clones."""
    state = [(t["p0"].to(dtype).clone(), torch.zeros_like(t["p0"], dtype=dtype), torch.zeros_like(t["p0"], dtype=dtype))
             for t in case]
    out = []
    for s in range(STEPS):
        for t, (p, m, v) in zip(case, state):
            sparse_adam_step(p, m, v, *t["steps"][s], s + 1)
        out.append([(p.clone(), m.clone(), v.clone()) for p, m, v in state])
    return out


def rel_err(got, want, per_row=False):
    """(max|got - want| / max|want|, that error, that scale) in float64 (0 / 0 = 0); per_row: of the
    row [.., dim] where the ratio is largest (a row whose want is all zero counts its error as it is)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    if not want.numel():
        return 0.0, 0.0, 0.0
    if not per_row:
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        return (err / scale if scale > 0 else err), err, scale
    err, scale = (got - want).abs().flatten(1).max(1).values, want.abs().flatten(1).max(1).values
    ratio = torch.where(scale > 0, err / scale.clamp_min(1e-300), err)
    r = int(ratio.argmax())
    return float(ratio[r]), float(err[r]), float(scale[r])


def err_of(kind, got, want):
    return rel_err(got, want, PER_ROW[kind])


def measure_drift():
    """Per tensor kind the largest rel_err of the float32 run against the float64 run, over all
    cases and steps."""
    worst = {k: 0.0 for k in REL}
    for name in CASES:
        case = make_case(name)
        for a, b in zip(run_case(case, torch.float32), run_case(case, torch.float64)):
            for ta, tb in zip(a, b):
                for k, x, y in zip(REL, ta, tb):
                    worst[k] = max(worst[k], err_of(k, x, y)[0])
    return worst
