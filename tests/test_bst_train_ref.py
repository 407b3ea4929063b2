"""CPU tests of tests/bst_train_ref.py, the float64 oracle of test_gpu_bst_train_ops.py.

First the oracle is tied to what the suite already trusts: its operations composed with F.linear are
oracle/reference_forward.py's bst_block_train (key-padding and dropout masks) and the pooling lines of
bst_forward_train, in float64 at 1e-12 relative; the closed-form backwards (LayerNorm, LeakyReLU +
dropout, pooling, position rows) are torch.autograd's gradients of the forwards.  Then the drift the
GPU tolerances rest on is measured: every compared tensor of every case of the GPU file's case table,
computed by the same restatement in float64 and in float32; per operation family the GPU file's
constant must be at least 50 x and at most 500 x the largest max|f32 - f64| / max|f64|."""
import pytest
import torch
import torch.nn.functional as F

import bst_train_ref as R
from oracle import reference_forward as ref
from test_gpu_bst_train_ops import REL

f64 = torch.float64


def close12(got, want, what):
    assert got.shape == want.shape and got.dtype == f64 and want.dtype == f64, what
    rel, err, scale = R.rel_err(got, want)
    assert rel <= 1e-12, f"{what}: {err:.3e} against max {scale:.3e}"


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=R.gen("bst_ref", shape, seed), dtype=f64)


def block_params(d, T):
    p = {}
    for k, n in enumerate(("w_q", "w_k", "w_v", "w_o", "ffn.0", "ffn.3")):
        p[f"b.{n}.weight"], p[f"b.{n}.bias"] = rnd(d, d, seed=k) / d ** 0.5, rnd(d, seed=10 + k)
    for k, n in enumerate(("norm1", "norm2")):
        p[f"b.{n}.weight"], p[f"b.{n}.bias"] = 1.0 + 0.5 * rnd(d, seed=20 + k), rnd(d, seed=30 + k)
    p["b.position_embedding.weight"] = rnd(T, d, seed=40)
    return p


@pytest.mark.parametrize("mean_pool", [False, True], ids=["sum", "mean"])
@pytest.mark.parametrize("dropout", [False, True], ids=["p0", "dropout"])
@pytest.mark.parametrize("B,T,d,heads", [(3, 5, 6, 2), (4, 20, 16, 4)])
def test_the_operations_compose_to_the_reference_train_block_and_pooling(B, T, d, heads, dropout, mean_pool):
    p = block_params(d, T)
    x = rnd(B * T, d, seed=50)
    lens = R.att_lens(B, T)
    g = R.gen("bst_ref masks", B, T, d)
    masks = [R.cpu_mask(g, (B * T, d), 0.25).double() for _ in range(3)] if dropout else [None] * 3
    lin = lambda t, n: F.linear(t, p[f"b.{n}.weight"], p[f"b.{n}.bias"])  # noqa: E731
    xp = R.add_pos(x, p["b.position_embedding.weight"], T)
    qkv = torch.cat([lin(xp, "w_q"), lin(xp, "w_k"), lin(x, "w_v")], 1)
    P, ctx = R.attention(qkv, B, T, d, heads, lens)
    r1, out1, _, _ = R.res_dropout_ln(xp, lin(ctx, "w_o"), masks[0], p["b.norm1.weight"], p["b.norm1.bias"], R.LN_EPS)
    a = R.leaky_dropout(lin(out1, "ffn.0"), masks[1], R.SLOPE)
    r2, out, _, _ = R.res_dropout_ln(out1, lin(a, "ffn.3"), masks[2], p["b.norm2.weight"], p["b.norm2.bias"], R.LN_EPS)
    x3 = x.view(B, T, d)
    padding = torch.arange(T).expand(B, T) >= lens.unsqueeze(1)
    want = ref.bst_block_train(p, "b.", x3, x3, x3, heads, padding, masks if dropout else None, eps=R.LN_EPS)
    close12(out.view(B, T, d), want, "block output")
    assert float(P[padding[:, None, None, :].expand_as(P)].abs().max()) == 0.0  # masked keys: exactly 0
    close12(P.sum(-1), torch.ones(B, heads, T, dtype=f64), "rows of P")
    # bst_forward_train's pooling lines (oracle/reference_forward.py)
    pooled = torch.sum(want, dim=1) / lens.unsqueeze(1).double() if mean_pool else torch.sum(want, dim=1)
    close12(R.pool(out, B, T, lens, mean_pool), pooled, "pooling")


@pytest.mark.parametrize("rows,d", [(5, 6), (7, 20), (3, 132)])
@pytest.mark.parametrize("dropout", [False, True], ids=["p0", "dropout"])
def test_ln_backward_is_autograd_of_res_dropout_ln(rows, d, dropout):
    i = R.ln_inputs((rows, d))
    mask = i.cpu_mask.double() if dropout else None
    base, o, gamma, beta = (R._leaf(t, f64) for t in (i.base, i.o, i.gamma, i.beta))
    r, y, mean, rstd = R.res_dropout_ln(base, o, mask, gamma, beta, R.LN_EPS)
    close12(y.detach(), F.layer_norm(r.detach(), (d,), gamma.detach(), beta.detach(), R.LN_EPS), "F.layer_norm")
    dbase, do, dgamma, dbeta = R._grads((y * i.dy.double()).sum(), [base, o, gamma, beta])
    got = R.ln_backward(i.dy.double(), r.detach(), mean.detach(), rstd.detach(), gamma.detach(), mask)
    for n, g, w in zip(("dr", "d_o", "dgamma", "dbeta"), got, (dbase, do, dgamma, dbeta)):
        close12(g, w, n)


@pytest.mark.parametrize("case", R.POOL_LN_CASES, ids=str)
def test_pooled_row_form_is_autograd_through_pooling_and_layer_norm(case):
    B, T, d, mean_pool = case
    i = R.pool_ln_inputs(case)
    mask = i.cpu_mask.double()
    base, o, gamma, beta = (R._leaf(t, f64) for t in (i.base, i.o, i.gamma, i.beta))
    r, y, mean, rstd = R.res_dropout_ln(base, o, mask, gamma, beta, R.LN_EPS)
    drow = i.drow[:, R.POOL_COL:R.POOL_COL + d].double()
    want = R._grads((R.pool(y, B, T, i.lens, mean_pool) * drow).sum(), [base, o, gamma, beta])
    got = R.pool_ln_backward(drow, T, i.lens, mean_pool, r.detach(), mean.detach(), rstd.detach(), gamma.detach(), mask)
    for n, g, w in zip(("dr", "d_o", "dgamma", "dbeta"), got, want):
        close12(g, w, n)


@pytest.mark.parametrize("case", R.LEAKY_CASES, ids=str)
def test_leaky_dropout_backward_is_autograd_and_f_leaky_relu(case):
    i = R.leaky_inputs(case)
    mask = None if i.cpu_mask is None else i.cpu_mask.double()
    want = R.leaky_eval(case, i, f64, mask)
    close12(R.leaky_dropout_backward(i.da.double(), i.f.double(), mask, R.SLOPE), want["df"], "df")
    close12(want["a"], F.leaky_relu(i.f.double(), R.SLOPE) * (1.0 if mask is None else mask), "F.leaky_relu")


def test_closed_forms_of_pooling_and_position_gradients_are_autograd():
    for case in R.POOL_BWD_CASES:
        B, T, d, mean = case
        i = R.pool_inputs(case)
        close12(R.pool_backward(i.drow[:, R.POOL_COL:R.POOL_COL + d].double(), T, i.lens, mean),
                R.pool_bwd_eval(case, i, f64)["dx"], f"pool_backward {case}")
    for case in R.POS_BWD_CASES:
        B, (T, d) = case
        i = R.pos_bwd_inputs(case)
        want = R.pos_bwd_eval(case, i, f64)["dpos"]
        close12(R.pos_backward(i.dxp.double(), B, T, i.dpos0[:T].double()), want[:T], f"pos_backward {case}")
        assert torch.equal(want[T], i.dpos0[T].double())  # the row past T gets no gradient


def test_gather_pos_zeroes_out_of_range_rows():
    table, pos = rnd(5, 4), rnd(3, 4, seed=1)
    idx = torch.tensor([0, -1, 4, 5, 2, 1, 3])
    x, xp = R.gather_pos(table, idx, pos, 3)
    bad = torch.tensor([False, True, False, True, False, False, False])
    assert torch.equal(x[~bad], table[idx[~bad]]) and float(x[bad].abs().max()) == 0.0
    assert torch.equal(xp, x + pos[torch.arange(7) % 3]) and torch.equal(xp[bad], pos[torch.tensor([1, 0])])


@pytest.mark.parametrize("case", [c for c in R.ATT_CASES if c[0] != R.LOOP], ids=R.att_id)
def test_the_score_gradients_rows_sum_to_zero_and_so_does_the_bias_gradient_of_w_k(case):
    """sum_j dS[i, j] = 0 in exact arithmetic, so dbk = sum_j dK[j] = sum_i (sum_j dS[i, j]) Q[i] is
    the oracle's own rounding noise: it has no usable max|want| and is compared on the scale of its
    summands (att_eval's "scale:dbk").  dbk is no output of the attention kernels (rk_linear's
    backward forms it from dK); dQ, dK and dV themselves are not such sums."""
    rc = R.att_resolve(case)
    want = R.att_eval(rc, R.att_inputs(rc), f64)
    ds = want["in:ds"]
    assert float(ds.sum(-1).abs().max()) <= 1e-12 * float(ds.abs().sum(-1).max())
    assert float(want["dbk"].abs().max()) <= 1e-12 * float(want["scale:dbk"])
    for n in ("dq", "dk", "dv") if case[1] > 1 else ("dv",):  # these have a scale of their own (T = 1: dS = 0)
        assert float(want[n].abs().max()) > 1e-3


def test_case_table_sequence_lengths_and_full_comparisons():
    """Every seq_len is in [1, T] (seq_len = 0 is a row of -inf: NaN in the oracle too, out of scope) and
    holds 1 and T; the looping cases' item counts are what their bounds ask for; every compared tensor
    has the operation's full shape, so no element is left out (LEAKY_EXCLUDED = 0: the LeakyReLU sign
    is taken from the same fp32 f on both sides)."""
    for c in R.ATT_CASES:
        B, T, d, heads = rc = R.att_resolve(c)
        lens = R.att_lens(B, T)
        assert lens.shape == (B,) and int(lens.min()) >= 1 and int(lens.max()) <= T
        assert 1 in lens.tolist() and T in lens.tolist()
        if B >= 12 and T > 17:
            assert {15, 16, 17} <= set(lens.tolist())
        if c[0] == R.LOOP:
            for bwd in (False, True):
                bound = R.NUM_CUS * min(8, (160 * 1024) // R.att_lds_bytes(T, d // heads, bwd))
                items = R.loop_batch(T, d, heads, R.NUM_CUS, bwd) * heads
                assert 2 * bound + 3 <= items < 2 * bound + 3 + heads and R.loop_batch(T, d, heads, R.NUM_CUS, bwd) <= B
    assert [R.att_slots(c[1], c[2] // c[3]) for c in R.ATT_CASES] == [0, 0, 0, 0, 1, 2, 2, 4, 4, 0]
    assert R.att_lds_bytes(64, 64, True) == 104 * 1024 - 2048 and R.att_lds_bytes(64, 64, False) == 51 * 1024
    assert [R.ln_lanes(d) for _, d in R.LN_CASES] == [8, 8, 8, 16, 16, 32, 32, 64, 64, 0, 0, 0, 8]
    rows, d = R.ln_resolve(R.LN_CASES[-1])
    groups = -(-rows // 8)
    assert -(-groups // 16) > 16 * R.NUM_CUS  # ceil(groups / 16) workgroups asked for: clamped
    assert R.LEAKY_EXCLUDED == 0
    for c in R.LEAKY_CASES:
        i = R.leaky_inputs(c)
        out = R.leaky_eval(c, i, f64, i.cpu_mask)
        assert out["a"].numel() == c[0] - R.LEAKY_EXCLUDED and out["df"].numel() == c[0] - R.LEAKY_EXCLUDED
        zeros = i.f[i.f == 0]
        assert bool(torch.signbit(zeros).any()) and (c[0] < 4 or not bool(torch.signbit(zeros).all()))
        assert c[0] < 4 or int((i.f < 0).sum()) >= 2
    rc = R.att_resolve(R.ATT_CASES[0])
    B, T, d, heads = rc
    out = R.att_eval(rc, R.att_inputs(rc), f64)
    assert out["P"].shape == (B, heads, T, T) and out["ctx"].shape == (B * T, d)
    assert all(out[n].shape == (B * T, d) for n in ("dq", "dk", "dv"))


def test_fp32_drift_of_the_case_table_bounds_the_gpu_tolerances(capsys):
    worst = {}
    for family, evals in R.family_evals().items():
        for cid, fn in evals:
            want, got = fn(torch.float64), fn(torch.float32)
            assert want.keys() == got.keys()
            for name in want:
                if ":" in name:
                    continue
                assert got[name].dtype == torch.float32 and want[name].dtype == f64, (family, cid, name)
                assert got[name].shape == want[name].shape
                rel = R.rel_err(got[name], want[name], want.get("scale:" + name))[0]
                if rel > worst.get(family, (-1.0,))[0]:
                    worst[family] = (rel, cid, name)
    with capsys.disabled():  # the table belongs in a plain run's output
        print(f"\n{'family':10s} {'fp32 drift':>11s} {'REL (GPU)':>10s}  worst case")
        for family, (rel, cid, name) in worst.items():
            print(f"{family:10s} {rel:11.3e} {REL[family]:10.1e}  {name} of {cid}")
    assert set(worst) == set(REL)
    for family, (rel, cid, name) in worst.items():
        assert rel <= REL[family] / R.MARGIN, f"{family}: drift {rel:.3e} > {REL[family]} / {R.MARGIN}"
        assert rel >= REL[family] / R.MARGIN / 10, f"{family}: REL {REL[family]} is over 500 x the drift {rel:.3e}"
