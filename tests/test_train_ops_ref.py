"""CPU tests of tests/train_ops_ref.py, the float64 oracle of test_gpu_train_ops.py.

First the oracle is tied to what the suite already trusts (oracle/reference_forward.py and
torch.nn.functional), in float64 at 1e-12 relative.  Then the drift the GPU tolerances rest on is
measured: every compared tensor of every case of the GPU file's case table, computed by the same
restatement in float64 and in float32; per operation family the largest max|f32 - f64| / max|f64|
must stay below the GPU file's constant divided by the margin (50), and above a tenth of that, so the
constant can be neither loosened nor left behind by a change of the case table unnoticed."""
import pytest
import torch
import torch.nn.functional as F

import train_ops_ref as R
from oracle import reference_forward as ref
from test_gpu_train_ops import REL

f64 = torch.float64


def close12(got, want, what):
    assert got.shape == want.shape and got.dtype == f64 and want.dtype == f64, what
    rel, err, scale = R.rel_err(got, want)
    assert rel <= 1e-12, f"{what}: {err:.3e} against max {scale:.3e}"


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=R.gen("ref", shape, seed), dtype=f64)


@pytest.mark.parametrize("B,N", [(2, 7), (5, 65), (130, 64)])
def test_dice_is_the_reference_dice_train(B, N):
    z, bias, alpha = rnd(B, N), rnd(N, seed=1), rnd(N, seed=2)
    p = {"d.alpha": alpha, "d.bn.running_mean": rnd(N, seed=3), "d.bn.running_var": rnd(N, seed=4).abs() + 0.5,
         "d.bn.num_batches_tracked": torch.zeros((), dtype=torch.int64)}
    rm, rv = p["d.bn.running_mean"].clone(), p["d.bn.running_var"].clone()
    want = ref.dice_train(z + bias, p, "d.", momentum=R.BN_MOMENTUM, eps=R.BN_EPS)
    y, mean, invstd, var, unbiased = R.dice(z, bias, alpha, R.BN_EPS)
    close12(y, want, "y")
    close12(R.BN_MOMENTUM * mean + (1 - R.BN_MOMENTUM) * rm, p["d.bn.running_mean"], "running_mean")
    close12(R.BN_MOMENTUM * unbiased + (1 - R.BN_MOMENTUM) * rv, p["d.bn.running_var"], "running_var")
    close12(invstd, 1.0 / torch.sqrt((z + bias).var(0, unbiased=False) + R.BN_EPS), "invstd")


@pytest.mark.parametrize("B,N", [(2, 7), (3, 64), (65, 130)])
@pytest.mark.parametrize("affine", [True, False])
def test_bn_act_is_torch_batch_norm(B, N, affine):
    z, bias = rnd(B, N), rnd(N, seed=1)
    gamma, beta = (rnd(N, seed=2), rnd(N, seed=3)) if affine else (None, None)
    rm, rv = rnd(N, seed=4), rnd(N, seed=5).abs() + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    want = F.batch_norm(z + bias, rm, rv, gamma, beta, training=True, momentum=R.BN_MOMENTUM, eps=R.BN_EPS)
    y, mean, invstd, var, unbiased = R.bn_act(z, bias, gamma, beta, R.BN_EPS, "none", 0.0, None)
    close12(y, want, "y")
    close12(R.BN_MOMENTUM * mean + (1 - R.BN_MOMENTUM) * rm0, rm, "running_mean")
    close12(R.BN_MOMENTUM * unbiased + (1 - R.BN_MOMENTUM) * rv0, rv, "running_var")
    mask = (rnd(B, N, seed=6) > 0).double() * 2.0
    close12(R.bn_act(z, bias, gamma, beta, R.BN_EPS, "leaky", 0.01, mask)[0], F.leaky_relu(want, 0.01) * mask, "leaky")
    close12(R.bn_act(z, bias, gamma, beta, R.BN_EPS, "relu", 0.0, None)[0], torch.relu(want), "relu")
    # without BN, and at B = 1 (which F.batch_norm refuses): the documented statistics
    close12(R.bn_act(z, bias, R.NO_BN, None, R.BN_EPS, "none", 0.0, None)[0], z + bias, "no bn")
    y1, mean1, invstd1, var1, unb1 = R.bn_act(z[:1], None, gamma, beta, R.BN_EPS, "none", 0.0, None)
    assert torch.equal(mean1, z[0]) and float(var1.abs().max()) == 0.0 and float(unb1.abs().max()) == 0.0
    close12(y1, (beta if affine else torch.zeros(N, dtype=f64)).expand(1, N), "B = 1")


@pytest.mark.parametrize("softmax", [False, True])
@pytest.mark.parametrize("shape", R.DIN_SHAPES, ids=str)
def test_din_pool_and_cross_compose_to_the_reference_attention(shape, softmax):
    B, T, H, A2 = shape
    i = R.din_inputs(shape)
    q, keys = i.q.double(), i.keys.double()
    w1, b1, w2, b2 = rnd(12, 4 * H, seed=1) / (4 * H) ** 0.5, rnd(12, seed=2), rnd(A2, 12, seed=3) / 12 ** 0.5, rnd(A2, seed=4)
    w3, b3 = i.w3.double(), i.b3.double()
    want = ref.din_attention(q, keys, i.lens, softmax, att=(w1, b1, w2, b2, w3.view(1, A2), b3))
    a2 = torch.relu(F.linear(torch.relu(F.linear(R.din_cross(q, keys), w1, b1)), w2, b2))
    w, out = R.din_pool(a2, w3, b3, keys, i.lens, softmax)
    close12(out, want, "attention output")
    past = torch.arange(T)[None, :] >= i.lens[:, None]
    if not softmax:
        assert float(w[past].abs().max()) == 0.0 if past.any() else True
    else:
        close12(w.sum(1), torch.ones(B, dtype=f64), "softmax rows")
        empty = i.lens == 0
        if empty.any():  # all T scores are the padding value: uniform weights
            close12(w[empty], torch.full_like(w[empty], 1.0 / T), "length 0")


@pytest.mark.parametrize("shape", R.AFM_SHAPES, ids=str)
def test_afm_pool_and_pairs_compose_to_the_reference_forward(shape):
    B, Fn, D, A, nd = shape
    i = R.afm_inputs(shape)
    names = [f"f{k}" for k in range(Fn)]
    w1, b1 = rnd(A, D, seed=1) / D ** 0.5, rnd(A, seed=2)
    p = {"dense_layer.weight": i.wd.double().view(1, nd), "dense_layer.bias": i.bd.double(),
         "attention.0.weight": w1, "attention.0.bias": b1, "attention.2.weight": i.w2.double().view(1, A),
         "attention.2.bias": i.b2.double(), "p.weight": i.wp.double().view(1, D), "p.bias": i.bp.double()}
    p.update({f"embeddings.{n}.weight": t.double() for n, t in zip(names, i.tables)})
    want_pred, want_total = ref.afm_forward(p, i.dense.double(), dict(zip(names, i.idx)), names)
    pairs = R.afm_pairs(i.emb.double())
    assert torch.equal(pairs.float(), i.pairs) and pairs.shape == (B, Fn * (Fn - 1) // 2, D)
    w, ws, logit, pred = R.afm_pool(torch.relu(F.linear(pairs, w1, b1)), i.w2.double(), i.b2.double(), pairs,
                                    i.dense.double(), i.wd.double(), i.bd.double(), i.wp.double(), i.bp.double())
    close12(logit, want_total.reshape(B), "total")
    close12(pred, want_pred.reshape(B), "pred")


def test_fm_second_and_combine_are_deepfm_terms():
    e = rnd(7, 26, 16)
    want = 0.5 * sum(e[:, a] * e[:, b] for a in range(26) for b in range(26) if a != b).sum(1)
    close12(R.fm_second(e), want, "fm second order")
    fm1, fm2, deep, w, b = rnd(7, seed=1), rnd(7, seed=2), rnd(7, seed=3), rnd(3, seed=4), rnd(1, seed=5)
    total, prob = R.fm_combine(fm1, fm2, deep, w, b)
    lin = F.linear(torch.stack([fm1, fm2, deep], 1), w.view(1, 3), b).reshape(7)
    close12(total, lin, "final_layer")
    close12(prob, torch.sigmoid(lin), "sigmoid")


def test_no_bn_pre_activation_of_the_case_table_is_near_zero():
    """test_gpu_train_ops.py compares every element of y and dz: no fp64 pre-activation of a BN case
    may be within rounding of zero (the issue allows 0.1 % of a case to be left out; the seeds leave
    out none)."""
    for c in R.BN_CASES:
        if not c[2]:
            continue
        i = R.bn_inputs(c)
        u = R.bn_pre(i.z.double(), None if i.bias is None else i.bias.double(), i.gamma.double(), i.beta.double(),
                     R.BN_EPS)[0]
        assert int(R.near_zero(u).sum()) == 0, R.bn_id(c)


def test_fp32_drift_of_the_case_table_bounds_the_gpu_tolerances(capsys):
    worst = {}
    for family, evals in R.family_evals().items():
        for cid, fn in evals:
            want, got = fn(torch.float64), fn(torch.float32)
            assert want.keys() == got.keys()
            for name in want:
                if name.startswith("scale:"):
                    continue
                assert got[name].dtype == torch.float32 and want[name].dtype == f64, (family, cid, name)
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
