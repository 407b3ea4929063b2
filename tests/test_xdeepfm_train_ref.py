"""CPU tests of the xDeepFM training restatement (tests/xdeepfm_train_ref.py) the GPU tests compare
against: the masked ReLU is torch.relu under the restatement's own sign, the gradient tolerance is
50 x the float32 drift measured here, and the pre-activations near ReLU's kink are rare enough for the
GPU tests' sign check to leave them out."""
import functools

import pytest
import torch

import helpers as H
import rankops
import xdeepfm_ref as X
import xdeepfm_train_ref as T

CASE_IDS = [c[0] for c in X.OP_CASES]


@functools.lru_cache(maxsize=None)
def reference(case, act):
    return T.op_grads(case, act, torch.float64)


@pytest.mark.parametrize("case", [X.OP_CASES[3], X.OP_CASES[1]], ids=["off_grid", "wechat_b7"])
def test_masked_relu_is_relu_under_its_own_sign(case):
    plain = reference(case, "relu")
    masked = T.op_grads(case, "relu", torch.float64, masks=[y > 0 for y in plain["pre"]])
    torch.testing.assert_close(masked["pooled"], plain["pooled"], atol=0, rtol=0)
    for (name, a), (_, b) in zip(T.grad_tensors(masked), T.grad_tensors(plain)):
        torch.testing.assert_close(a, b, atol=0, rtol=0, msg=name)
    ident = reference(case, "identity")
    assert not torch.equal(ident["dx0"], plain["dx0"])  # the mask bites
    # and the restatement's forward is xdeepfm_ref's
    torch.testing.assert_close(plain["pooled"], X.op_reference(case, "relu")[0], atol=1e-12, rtol=1e-12)


def measured_drift():
    """(largest drift, where) of the restatement in float32 against float64, per gradient tensor, over
    xdeepfm_ref.OP_CASES with both activations and the full loss.  Both runs use the float64 run's
    activation pattern, as the GPU tests hand one pattern to both sides.  T.SLAB_CASE is left out: see
    the note on GRAD_TOL in tests/xdeepfm_train_ref.py."""
    worst, where = 0.0, None
    for case in X.OP_CASES:
        for act in X.ACTIVATIONS:
            r64 = reference(case, act)
            r32 = T.op_grads(case, act, torch.float32, masks=[y > 0 for y in r64["pre"]])
            for (name, a), (_, b) in zip(T.grad_tensors(r32), T.grad_tensors(r64)):
                d = T.grad_err(a, b)
                print(f"{case[0]:12s} {act:9s} {name:8s} drift {d:.3g}")
                if d > worst:
                    worst, where = d, (case[0], act, name)
    return worst, where


def test_grad_tolerance_is_50x_the_measured_fp32_drift():
    drift, where = measured_drift()
    print(f"largest fp32 gradient drift {drift:.3g} at {where}")
    assert 25 * drift <= T.GRAD_TOL <= 100 * drift, (T.GRAD_TOL, drift, where)


@pytest.mark.parametrize("case", T.GPU_OP_CASES, ids=[c[0] for c in T.GPU_OP_CASES])
def test_near_kink_share_is_small(case):
    r64 = reference(case, "relu")
    r32 = T.op_grads(case, "relu", torch.float32)
    band = sum(int(T.near_kink(y).sum()) for y in r64["pre"])
    total = sum(y.numel() for y in r64["pre"])
    flips = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(r32["pre"], r64["pre"]))
    smallest = min(float(y.abs().min()) for y in r64["pre"])
    print(f"{case[0]}: near-kink share {band / total:.3g}, float32 sign flips {flips}, min |y| {smallest:.3g}")
    assert band / total <= T.NEAR_KINK_MAX
    # a float32 flip can only happen inside the band
    for a, b in zip(r32["pre"], r64["pre"]):
        assert bool(T.near_kink(b)[(a > 0) != (b > 0)].all())


def test_forward_train_is_the_eval_restatement_without_batchnorm_and_dropout():
    small = {f: H.SMALL_VOCAB[f] for f in rankops.deepfm.WECHAT_FIELDS}
    torch.manual_seed(42)
    m = rankops.XDeepFM(None, cin_activation="relu", batch_norm=False, dropout_rate=0.0, vocab_sizes=small)
    p = X.floats(H.cpu_params(m), torch.float64)
    cat = H.deepfm_inputs(9, small, 9)["category"]
    got = T.forward_train(p, cat, "relu", batch_norm=False, dropout_rate=0.0)
    for a, b in zip(got, X.forward(p, cat, "relu")):
        torch.testing.assert_close(a, b, atol=1e-12, rtol=1e-12)
