"""CPU checks of tests/esmm_ref.py, the restatement the GPU tests of ESMM compare against: it is tied to an
independent per-row loop and to mmoe_ref's towers, its analytic loss gradient to float64 autograd, its
tolerance constants to the float32 drift they are derived from, and its seeded cases are shown to be
able to expose an error."""
import math

import pytest
import torch
import torch.nn.functional as F

import esmm_ref as R
import helpers as H
import mmoe_ref as M
import rankops

ORDINARY = [c for c in R.OP_CASES if c[0] != R.SATURATED]


def test_restatement_equals_a_per_row_loop():
    g = torch.Generator().manual_seed(5)
    B, width, K, units = 3, 5, 3, (4, 3)
    x = torch.randn(B, width, generator=g, dtype=torch.float64)
    towers = []
    for _ in range(K):
        hidden, last = M._stack_inputs(g, width, units)
        towers.append((hidden, M._linear(g, 1, last, 4.0)))
    towers = R.cast(towers, torch.float64)
    probs, logits, cond = R.esmm(x, towers)
    for b in range(B):
        run = 1.0
        for k, (hidden, (w, bias)) in enumerate(towers):
            h = [float(v) for v in x[b]]
            for W, bb in hidden:
                h = [max(0.0, sum(float(W[n, j]) * h[j] for j in range(len(h))) + float(bb[n])) for n in range(W.shape[0])]
            z = sum(float(w[0, j]) * h[j] for j in range(len(h))) + float(bias[0])
            c = 1.0 / (1.0 + math.exp(-z))
            run *= c
            assert abs(float(logits[b, k]) - z) < 1e-12
            assert abs(float(cond[b, k]) - c) < 1e-12 and abs(float(probs[b, k]) - run) < 1e-12
    assert torch.equal(probs[:, 0], cond[:, 0])


def test_a_tower_is_mmoe_refs_stack():
    c = R.case("odd")
    rows, towers = R.op_inputs(c)
    x = rows[:, :c[1]].double()
    hidden, (w, b) = R.cast(towers, torch.float64)[1]
    want = M.linear(M.stack(x, hidden), w, b.reshape(1, 1))
    assert torch.equal(R.esmm(x, R.cast(towers, torch.float64))[1][:, 1:2], want)
    ordered = R.esmm(rows[:, :c[1]], towers, ordered=True)[1]
    assert R.rel_err(ordered, R.op_reference(c)[1]) < 1e-5


def test_loss_equals_a_per_row_loop():
    lc = (17, 3, 2.0, (1.0, 0.5, 2.0))
    zb, yb = R.loss_inputs(lc)
    z, y = zb[:, :3].double(), yb[:, :3].double()
    loss, per_task, _ = R.loss(z, y, lc[3])
    total = [0.0, 0.0, 0.0]
    for b in range(17):
        p = 1.0
        for k in range(3):
            p *= 1.0 / (1.0 + math.exp(-float(z[b, k])))
            yk = float(y[b, k])
            total[k] += -(yk * math.log(p) + (1 - yk) * math.log(1 - p))
    for k in range(3):
        assert abs(float(per_task[k]) - total[k] / 17) < 1e-12
    assert abs(float(loss) - sum(w * t / 17 for w, t in zip(lc[3], total))) < 1e-12
    assert bool((yb[:, 1:3] <= yb[:, 0:2]).all())  # nested labels


def test_analytic_gradient_equals_float64_autograd():
    for lc in ((17, 2, 2.0, None), (64, 8, 2.0, None), (300, 3, 2.0, (1.0, 0.5, 2.0))):
        zb, yb = R.loss_inputs(lc)
        K = lc[1]
        z = zb[:, :K].double().requires_grad_(True)
        y = yb[:, :K].double()
        w = torch.ones(K, dtype=torch.float64) if lc[3] is None else torch.tensor(lc[3], dtype=torch.float64)
        S = torch.cumsum(F.logsigmoid(z), dim=1)
        L = -(y * S + (1 - y) * torch.log1p(-torch.exp(S)))
        (L.sum(dim=0) / lc[0] * w).sum().backward()
        loss, _, g = R.loss(z.detach(), y, lc[3])
        err = float((g - z.grad).abs().max()) * lc[0]
        print(f"{lc}: analytic vs autograd {err:.3g}")
        assert err < 1e-12


def test_loss_is_finite_at_extreme_logits():
    z = torch.tensor([[200.0, 200.0, 200.0], [-200.0, 200.0, -200.0], [200.0, -200.0, 200.0]])
    y = torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    for out in R.loss(z, y):
        assert bool(torch.isfinite(out).all())


def test_module_creation_order_and_keys():
    torch.manual_seed(42)
    esmm = rankops.ESMM(None, vocab_sizes=H.SMALL_VOCAB)
    torch.manual_seed(42)
    mmoe = rankops.MMoE(None, vocab_sizes=H.SMALL_VOCAB)
    keys = list(esmm.state_dict())
    emb = [k for k in keys if k.startswith("embeddings.")]
    assert keys[:len(emb)] == emb == [k for k in mmoe.state_dict() if k.startswith("embeddings.")]
    rest = keys[len(emb):]
    want = [f"towers.{k}.{i}.{n}" for k in range(2) for i in (0, 3, 6) for n in ("weight", "bias")]
    want += [f"tower_outputs.{k}.{n}" for k in range(2) for n in ("weight", "bias")]
    assert rest == want
    for k in emb:  # the same seed gives the same tables
        assert torch.equal(esmm.state_dict()[k], mmoe.state_dict()[k])
    other = rankops.ESMM(None, vocab_sizes=H.SMALL_VOCAB)
    missing = other.load_state_dict({k: v for k, v in mmoe.state_dict().items() if k.startswith("embeddings.")},
                                    strict=False)
    assert not missing.unexpected_keys and all(not k.startswith("embeddings.") for k in missing.missing_keys)
    assert torch.equal(other.embeddings["userid"].weight, mmoe.embeddings["userid"].weight)
    for flags in (dict(trainable=True), dict(trainable=True, sparse_grad=True)):
        torch.manual_seed(42)
        flagged = rankops.ESMM(None, vocab_sizes=H.SMALL_VOCAB, **flags)
        assert list(flagged.state_dict()) == keys
        assert all(torch.equal(a, b) for a, b in zip(flagged.state_dict().values(), esmm.state_dict().values()))
    assert esmm.fits() and len(list(esmm.towers[0])) == 9  # Linear, ReLU, Dropout per unit
    for bad in (dict(task_names=("click",)), dict(tower_hidden_units=()), dict(task_names=("a", "a"))):
        with pytest.raises(ValueError):
            rankops.ESMM(None, vocab_sizes=H.SMALL_VOCAB, **bad)
    assert not rankops.common.esmm_fits(50, 7, 9, (64,)) and not rankops.common.esmm_fits(50, 7, 2, (513,))
    assert not rankops.common.esmm_fits(50, 7, 2, (8, 8, 8, 8)) and rankops.common.esmm_fits(256, 16, 8, (512, 512, 512))


def test_tolerances_are_50x_the_float32_drift():
    measured = R.drifts()
    consts = {"ordinary": (R.LOGIT_TOL, R.PROB_TOL, R.COND_TOL),
              "saturated": (R.SAT_LOGIT_TOL, R.SAT_PROB_TOL, R.SAT_COND_TOL),
              "loss": (R.LOSS_TOL, R.TASK_LOSS_TOL, R.DLOGIT_TOL),
              "sat_loss": (R.SAT_LOSS_TOL, R.SAT_TASK_LOSS_TOL, R.SAT_DLOGIT_TOL)}
    for which, tols in consts.items():
        for tol, drift in zip(tols, measured[which]):
            print(f"{which}: drift {drift:.3g}, constant {tol:.3g} = {tol / drift:.1f} x")
            assert 25 * drift <= tol <= 100 * drift, (which, drift, tol)


@pytest.mark.parametrize("c", ORDINARY, ids=[c[0] for c in ORDINARY])
def test_ordinary_cases_cannot_hide_an_error(c):
    name, width, K, tu, B = c
    clipped = []
    R.op_reference(c, clipped=clipped)
    probs, logits, cond = R.op_reference(c)
    half = (B + 1) // 2
    for i in range(K):
        for j in range(i):  # a kernel reading tower j's weights for tower i fails
            assert int(((logits[:, i] - logits[:, j]).abs() > 100 * R.LOGIT_TOL).sum()) >= half, (name, i, j)
    for k in range(1, K):   # a product that drops its last factor fails
        assert int(((probs[:, k] - probs[:, k - 1]).abs() > 100 * R.PROB_TOL).sum()) >= half, (name, k)
    assert max(clipped) <= 0.9, (name, clipped)


def test_saturated_case_saturates_in_both_directions():
    probs, logits, _ = R.op_reference(R.case(R.SATURATED))
    assert int((probs > 1 - 1e-6).any(dim=1).sum()) >= 8 and int((probs < 1e-6).any(dim=1).sum()) >= 8
    assert 20 <= float(logits.max()) <= 30 and -30 <= float(logits.min()) <= -20


def test_naive_float32_loss_is_why_the_kernel_exists():
    """On saturated logits float32 BCE of the product of sigmoids (torch clamps its logs at -100 and 1 - pq
    loses the small factor) and its autograd gradient miss float64 by more than 1000 x the tolerances the
    log-domain formulation is held to."""
    lc = R.LOSS_CASES[2]
    assert lc[:3] == (300, 3, 8.0)
    zb, yb = R.loss_inputs(lc)
    z = zb[:, :3].clone().requires_grad_(True)
    y = yb[:, :3]
    w = torch.tensor(lc[3])
    naive = (F.binary_cross_entropy(torch.cumprod(torch.sigmoid(z), dim=1), y, reduction="none").mean(dim=0) * w).sum()
    naive.backward()
    ref_loss, _, ref_g = R.loss_reference(lc)
    loss_err = R.rel_err(naive.detach(), ref_loss)
    grad_err = R.rel_err(z.grad * lc[0], ref_g * lc[0])
    print(f"naive float32: loss err {loss_err:.3g}, gradient err {grad_err:.3g}")
    assert loss_err > 1000 * R.SAT_LOSS_TOL and grad_err > 1000 * R.SAT_DLOGIT_TOL
