"""CPU checks of tests/esmm_train_ref.py: without dropout it is esmm_ref bit for bit, its joint-gradient
helper matches the formula rk_esmm_joint_backward implements, and its gradient tolerances are 50 x the
float32 drift they are derived from."""
import torch

import esmm_ref as R
import esmm_train_ref as T


def test_without_dropout_it_is_esmm_ref_bit_for_bit():
    for c in (R.case("odd"), R.case("chain8")):
        rows, towers = R.op_inputs(c)
        x = rows[:, :c[1]]
        for dtype, ordered in ((torch.float64, False), (torch.float32, True)):
            a = T.esmm(x.to(dtype), R.cast(towers, dtype), None, ordered)
            b = R.esmm(x.to(dtype), R.cast(towers, dtype), ordered=ordered)
            assert all(torch.equal(u, v) for u, v in zip(a, b))
    mc = R.MODEL_CASES[1]
    p = R.floats(R.build_model(mc).state_dict(), torch.float64)
    inp = R.model_inputs(mc)
    a, b = T.forward(p, **inp), R.forward(p, **inp)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_dropout_multipliers_reach_the_output():
    c = R.case("odd")
    rows, towers = R.op_inputs(c)
    x = rows[:, :c[1]].double()
    keeps = T.cpu_keeps(T.sites_of(c[2], c[3]), c[4], 0.5)
    a = T.esmm(x, R.cast(towers, torch.float64), keeps)
    b = T.esmm(x, R.cast(towers, torch.float64))
    assert not torch.equal(a[1], b[1])
    assert [s for s, _ in T.sites_of(3, (24, 7))] == [0, 1, 2, 3, 4, 5]


def test_joint_gradient_formula():
    z = R.loss_inputs(R.LOSS_CASES[4])[0][:, :8].double()
    for use in (("probs",), ("logits",), ("cond",), ("probs", "logits", "cond")):
        inc, ref = T.joint_gradients(z, use)
        probs, cond = R.chain(z)
        sn = torch.sigmoid(-z)
        g = torch.zeros_like(z)
        if "logits" in inc:
            g = g + inc["logits"]
        if "cond" in inc:
            g = g + cond * sn * inc["cond"]
        if "probs" in inc:
            tail = torch.flip(torch.cumsum(torch.flip(inc["probs"] * probs, [1]), dim=1), [1])
            g = g + sn * tail
        assert float((g - ref).abs().max()) < 1e-12, use


def test_tolerances_are_50x_the_float32_drift():
    for name, tol, drift in zip(("dx", "dw", "joint"), (T.DX_TOL, T.DW_TOL, T.JOINT_TOL), T.drifts()):
        print(f"{name}: drift {drift:.3g}, constant {tol:.3g} = {tol / drift:.1f} x")
        assert 25 * drift <= tol <= 100 * drift, (name, drift, tol)
