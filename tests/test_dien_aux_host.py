"""CPU tests of DIEN's auxiliary loss: the module's flags and parameters, the float64 restatement
(tests/dien_aux_ref.py) the GPU tests are judged by, and the tolerances those tests import.

Tolerances (test_tolerances_are_fifty_times_the_fp32_drift): the restatement differentiated in
float32 on the CPU against float64, over the GPU test's shapes, both cells, T_neg in {1, 3}, the
loss alone on given states and the composition with the interest recurrence.  Worst drift relative
to each tensor's largest float64 entry, as printed by this test: 2.3e-7 for the loss (per-sample,
mean and the composition's scalar) and 1.4e-6 for a gradient tensor (the composition's dA on the
3x3x8x8 AGRU case, dq 1.2e-6 next; the loss alone stays below 6e-7, its dw_aux on 5x200x32x16).
Fifty times those, the convention of test_gpu_dien_train.py for hardware exp / rcp and another
summation order, are 1.2e-5 and 6.9e-5; rounded up so that another CPU's float32 summation order
does not trip the assertion here: REL_LOSS = 2e-5, REL_GRAD = 1e-4.  A dropped mask, an off-by-one
pairing or a wrong sign shows at 1e-1 and more."""
import inspect

import pytest
import torch

import dien_aux_ref as R
import helpers as H
import rankops


def _model(seed=5, **kw):
    torch.manual_seed(seed)
    return rankops.DIEN(None, hidden_units=[16, 8], vocab_sizes=H.SMALL_VOCAB, **kw)


def test_constructor_flags_are_keyword_only_with_the_reference_defaults():
    sig = inspect.signature(rankops.DIEN.__init__).parameters
    for name, default in (("use_auxiliary_loss", False), ("negative_sample_number", 3)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert sig[name].default == default, name
    with pytest.raises(TypeError):
        rankops.DIEN(None, [16], "dice", 0.1, True, "AGRU", 8, True)  # no ninth positional argument
    with pytest.raises(ValueError):
        _model(use_auxiliary_loss=True, negative_sample_number=0)


def test_flag_off_model_is_the_parent_model_and_flag_on_adds_one_parameter():
    plain, off, on = _model(), _model(use_auxiliary_loss=False), _model(use_auxiliary_loss=True)
    sp, so, sn = plain.state_dict(), off.state_dict(), on.state_dict()
    assert list(sp) == list(so) and "aux_project_matrix" not in so
    for k in sp:
        assert torch.equal(sp[k], so[k]), k
    assert set(sn) - set(sp) == {"aux_project_matrix"} and set(sp) <= set(sn)
    assert tuple(sn["aux_project_matrix"].shape) == (16, 8)  # [H, nh], dien.py:268
    for k in sp:  # drawn last: every other parameter starts where the default model's does
        assert torch.equal(sp[k], sn[k]), k
    # the random stream a default model consumes is unchanged
    torch.manual_seed(9)
    rankops.DIEN(None, hidden_units=[16, 8], vocab_sizes=H.SMALL_VOCAB)
    x = torch.rand(4)
    torch.manual_seed(9)
    rankops.DIEN(None, hidden_units=[16, 8], vocab_sizes=H.SMALL_VOCAB, use_auxiliary_loss=False)
    assert torch.equal(x, torch.rand(4))
    bound = (6.0 / (16 + 8)) ** 0.5  # Glorot uniform
    w = sn["aux_project_matrix"]
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.5 * bound
    assert plain.use_auxiliary_loss is False and plain.negative_sample_number == 3


def _inputs(B, T, Hd, nh, T_neg, seed=3):
    g = torch.Generator().manual_seed(seed)
    hs = torch.rand(B, T, nh, generator=g, dtype=torch.float64) * 2 - 1
    keys = torch.randn(B, T, Hd, generator=g, dtype=torch.float64)
    neg = torch.randn(B, (T - 1) * T_neg, Hd, generator=g, dtype=torch.float64)
    w_aux = torch.rand(Hd, nh, generator=g, dtype=torch.float64) - 0.5
    return hs, keys, neg, w_aux


def test_loss_is_exactly_zero_without_a_step():
    hs, keys, neg, w_aux = _inputs(3, 1, 8, 8, 2)
    mean, per = R.aux_loss(hs, keys, neg, torch.tensor([0, 1, 1]), w_aux)
    assert float(mean) == 0.0 and float(per.abs().max()) == 0.0
    hs, keys, neg, w_aux = _inputs(4, 6, 8, 8, 2)
    lens = torch.tensor([0, 1, 6, 3])
    mean, per = R.aux_loss(hs, keys, neg, lens, w_aux)
    assert float(per[0]) == 0.0 and float(per[1]) == 0.0 and float(per[2]) > 0.0 and float(per[3]) > 0.0
    assert float(mean) == pytest.approx(float(per.sum()) / 4, rel=1e-15)


def test_masked_positions_get_exactly_zero_gradient():
    B, T, Hd, nh, T_neg = 5, 7, 8, 8, 3
    hs, keys, neg, w_aux = [t.requires_grad_(True) for t in _inputs(B, T, Hd, nh, T_neg)]
    lens = torch.tensor([0, 1, 2, 7, 4])
    R.aux_loss(hs, keys, neg, lens, w_aux)[0].backward()
    t = torch.arange(T)[None, :]
    dead_key = (t == 0) | (t >= lens[:, None])          # row 0 is never a "next behaviour"
    dead_h = t >= lens[:, None] - 1
    dead_neg = (torch.arange(T - 1)[None, :] >= lens[:, None] - 1).repeat_interleave(T_neg, 1)
    assert float(keys.grad[dead_key].abs().max()) == 0.0 and float(keys.grad[~dead_key].abs().min()) > 0.0
    assert float(hs.grad[dead_h].abs().max()) == 0.0
    assert float(neg.grad[dead_neg].abs().max()) == 0.0 and float(neg.grad[~dead_neg].abs().max()) > 0.0


@pytest.mark.parametrize("T_neg", [1, 3])
def test_restatement_agrees_with_the_literal_loop(T_neg):
    hs, keys, neg, w_aux = _inputs(4, 6, 8, 8, T_neg)
    lens = torch.tensor([6, 2, 1, 0])
    mean, per = R.aux_loss(hs, keys, neg, lens, w_aux)
    lmean, lper = R.aux_loss_loop(hs, keys, neg, lens, w_aux)
    torch.testing.assert_close(per, lper, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(mean, lmean, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("T_neg", [1, 3])
def test_restatement_is_the_sign_flipped_reference_expression(T_neg):
    hs, keys, neg, w_aux = _inputs(4, 6, 8, 8, T_neg)  # mild: |dot| stays below ~10
    lens = torch.tensor([6, 2, 1, 0])
    mean, _ = R.aux_loss(hs, keys, neg, lens, w_aux)
    want = R.aux_loss_reference_form(hs, keys, neg, lens, w_aux)
    torch.testing.assert_close(mean, want, rtol=1e-12, atol=1e-12)
    assert float(mean) > 0.0  # a loss: the reference's own sign would be negative
    # and where log(sigmoid(x)) overflows, log_sigmoid does not
    x = torch.tensor([-800.0, 800.0], dtype=torch.float64)
    assert torch.isinf(torch.log(torch.sigmoid(x)))[0] and torch.equal(R.log_sigmoid(x), torch.tensor([-800.0, 0.0],
                                                                                                      dtype=torch.float64))


def _drift(got, want):
    """max |got - want| / max |want|; a tensor the oracle leaves empty, untouched or all zero must be
    so in float32 too."""
    if want is None or want.numel() == 0 or float(want.abs().max()) == 0.0:
        assert got is None or got.numel() == 0 or float(got.abs().max()) == 0.0
        return 0.0
    return float((got.double() - want).abs().max()) / float(want.abs().max())


def test_tolerances_are_fifty_times_the_fp32_drift():
    worst_loss, worst_grad, where = 0.0, {}, {}
    for shape in R.SHAPES:
        for cell in R.CELLS:
            for T_neg in R.T_NEGS:
                _, m64, p64, g64 = R.op_oracle(*shape, T_neg, cell)
                _, m32, p32, g32 = R.op_oracle(*shape, T_neg, cell, dtype=torch.float32)
                l64, c64 = R.composition_oracle(*shape, T_neg, cell)
                l32, c32 = R.composition_oracle(*shape, T_neg, cell, dtype=torch.float32)
                worst_loss = max(worst_loss, _drift(m32, m64), _drift(p32, p64), _drift(l32, l64))
                for names, a, b, tag in ((R.OP_NAMES, g32, g64, "op"), (R.COMP_NAMES, c32, c64, "comp")):
                    for n, x, y in zip(names, a, b):
                        d = _drift(x, y)
                        if d > worst_grad.get(f"{tag}.{n}", 0.0):
                            worst_grad[f"{tag}.{n}"], where[f"{tag}.{n}"] = d, (shape, cell, T_neg)
    print(f"worst loss drift {worst_loss:.3e}")
    for n, d in worst_grad.items():
        print(f"worst drift {n}: {d:.3e} at {where[n]}")
    assert 50 * worst_loss <= R.REL_LOSS, worst_loss
    assert 50 * max(worst_grad.values()) <= R.REL_GRAD, worst_grad
