"""The MMoE training restatement (tests/mmoe_train_ref.py) checked on the CPU: it is mmoe_ref in eval, its
autograd gradients agree with the written-out backward and with finite differences, its tolerance constants
sit inside 25-100 x of the drifts they come from, and its seeded cases cannot hide a failure."""
import pytest
import torch

import helpers as H
import mmoe_ref as R
import mmoe_train_ref as T


def test_eval_is_mmoe_ref_exactly():
    for c in T.GRAD_CASES:
        rows, experts, gates, towers = T.op_inputs(c)
        x = rows[:, :c[1]].double()
        a = R.mmoe(x, R.cast(experts, torch.float64), R.cast(gates, torch.float64), R.cast(towers, torch.float64))
        b = T.mmoe(x, R.cast(experts, torch.float64), R.cast(gates, torch.float64), R.cast(towers, torch.float64))
        assert all(torch.equal(p, q) for p, q in zip(a, b)), c[0]
    model = T.build_model(R.ALT_CONFIG).eval()
    p = R.floats(H.cpu_params(model), torch.float64)
    dense, cat = T.model_inputs(17)
    assert all(torch.equal(u, v) for u, v in zip(R.forward(p, dense, cat), T.forward(p, dense, cat)))


def test_gradients_agree_with_the_written_out_backward_row_by_row():
    """One expert layer, no towers, loss = sum(c_m mixed): the mix / softmax backward as
    rk_mmoe_mix_backward states it, one row at a time."""
    c = ("tiny", 5, 3, 2, (4,), (), 6)
    rows, experts, gates, _ = T.op_inputs(c)
    x = rows[:, :5].double()
    ex, ga = R.cast(experts, torch.float64), R.cast(gates, torch.float64)
    keeps = T.cpu_keeps(T.sites_of(3, 2, (4,), ()), 6, 0.25)
    ref = T.op_gradients(x, ex, ga, None, keeps=keeps, use=("mixed",))
    mixed, g = ref["out"]
    cm = T.loss_coeffs(6, 2, 4)[0]
    dx = torch.zeros_like(x)
    dW = [torch.zeros_like(l[0][0]) for l in ex]
    db = [torch.zeros_like(l[0][1]) for l in ex]
    dWg = [torch.zeros_like(w) for w, _ in ga]
    dbg = [torch.zeros_like(b) for _, b in ga]
    for r in range(6):
        f = [torch.relu(ex[e][0][0] @ x[r] + ex[e][0][1]) * keeps[e][r] for e in range(3)]
        for k in range(2):
            dg = torch.stack([cm[r, k] @ f[e] for e in range(3)])
            dgl = g[r, k] * (dg - (g[r, k] * dg).sum())
            dWg[k] += torch.outer(dgl, x[r])
            dbg[k] += dgl
            dx[r] += dgl @ ga[k][0]
        for e in range(3):
            dz = sum(g[r, k, e] * cm[r, k] for k in range(2)) * (f[e] > 0) * keeps[e][r]
            dW[e] += torch.outer(dz, x[r])
            db[e] += dz
            dx[r] += dz @ ex[e][0][0]
    torch.testing.assert_close(ref["dx"], dx, rtol=1e-12, atol=1e-12)
    for e in range(3):
        torch.testing.assert_close(ref["experts"][2 * e], dW[e], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(ref["experts"][2 * e + 1], db[e], rtol=1e-12, atol=1e-12)
    for k in range(2):
        torch.testing.assert_close(ref["gates"][2 * k], dWg[k], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(ref["gates"][2 * k + 1], dbg[k], rtol=1e-12, atol=1e-12)


def test_gradcheck_on_a_tiny_shape():
    c = ("tiny", 4, 2, 2, (3, 3), (2,), 3)
    rows, experts, gates, towers = T.op_inputs(c)
    leaves = T.flat(T.leaves((rows[:, :4], experts, gates, towers), torch.float64))
    keeps = T.cpu_keeps(T.sites_of(2, 2, (3, 3), (2,)), 3, 0.25)

    def fn(*ts):
        it = iter(ts)
        x = next(it)
        ex = [[(next(it), next(it)) for _ in range(2)] for _ in range(2)]
        ga = [(next(it), next(it)) for _ in range(2)]
        tw = [([(next(it), next(it))], (next(it), next(it))) for _ in range(2)]
        m, _, logits, probs = T.mmoe(x, ex, ga, tw, keeps)
        return m, logits, probs
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-5)


def test_tolerances_sit_inside_their_band():
    d = T.drifts()
    consts = {"ordinary": (T.DX_TOL, T.DW_TOL, T.DGATE_TOL),
              "extreme": (T.EXTREME_DX_TOL, T.EXTREME_DW_TOL, T.EXTREME_DGATE_TOL)}
    for which in d:
        for name, drift, const in zip(("dx", "dw", "dgate"), d[which], consts[which]):
            print(f"{which} {name}: drift {drift:.3e}, constant {const:.1e} = {const / drift:.1f} x")
            assert 25 * drift <= const <= 100 * drift, (which, name, drift, const)


# the gate-logit gradients must not be negligible next to dmixed (N(0, 1) coefficients: scale 1), or a wrong
# softmax backward would pass inside the tolerance's absolute part: the largest gate weight gradient of
# every ordinary case with more than one expert is at least GATE_GRAD_FLOOR
GATE_GRAD_FLOOR = 0.05


def test_seeded_cases_cannot_hide_a_failure():
    for c in T.GRAD_CASES:
        rows, experts, gates, towers = T.op_inputs(c)
        clipped = []
        T.mmoe(rows[:, :c[1]].double(), R.cast(experts, torch.float64), R.cast(gates, torch.float64),
               R.cast(towers, torch.float64), clipped=clipped)
        print(f"{c[0]}: ReLU clipping {min(clipped):.3f}-{max(clipped):.3f}")
        assert all(0.2 <= v <= 0.8 for v in clipped), (c[0], clipped)  # every ReLU, as test_mmoe_ref.py
        if c[2] > 1 and c[0] != R.EXTREME:
            top = max(float(g.abs().max()) for g in T.op_reference(c)["gates"])
            print(f"{c[0]}: largest gate gradient {top:.3e} (floor {GATE_GRAD_FLOOR})")
            assert top >= GATE_GRAD_FLOOR, (c[0], top)
    for name, B, kw in T.MODEL_CASES:
        model = T.build_model(kw)
        sites = T.sites_of(model.num_experts, len(model.task_names), model.expert_hidden_units, model.tower_hidden_units)
        for s, k in T.cpu_keeps(sites, B, T.DROPOUT_P).items():
            assert abs(float((k > 0).double().mean()) - (1 - T.DROPOUT_P)) <= 0.1, (name, s)


def test_flags_add_no_parameter_and_draw_nothing():
    a, b = T.build_model({}), T.build_model({}, trainable=True, sparse_grad=True)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert b.trainable and b.sparse_grad and not a.trainable and not a.sparse_grad
