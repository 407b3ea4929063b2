"""CPU tests of the xDeepFM restatement (tests/xdeepfm_ref.py) the GPU tests compare against: it is
tied to an independent triple-loop reading of the paper's eq. 6 and to the oracle's DeepFM, the
module's creation order and keys are the definition's, and the tolerance constants are 50 x the
float32 drift measured here."""
import pytest
import torch

import helpers as H
import rankops
import xdeepfm_ref as X
from oracle import reference_forward as ref

SMALL = {f: H.SMALL_VOCAB[f] for f in rankops.deepfm.WECHAT_FIELDS}  # the six wechat fields


def loop_cin(x0, Ws, bs, act):
    """Eq. 6 read literally: every (b, n, d) by its own sum over (h, i)."""
    f = X.act_fn(act)
    B, m, D = x0.shape
    xk, pooled = x0, []
    for W, b in zip(Ws, bs):
        Hk, Hp = W.shape[0], xk.shape[1]
        nxt = torch.zeros(B, Hk, D, dtype=x0.dtype)
        for bb in range(B):
            for n in range(Hk):
                for d in range(D):
                    acc = 0.0
                    for h in range(Hp):
                        for i in range(m):
                            acc += float(W[n, h * m + i]) * float(xk[bb, h, d]) * float(x0[bb, i, d])
                    nxt[bb, n, d] = acc + float(b[n])
        xk = f(nxt)
        pooled.append(xk.sum(dim=2))
    return torch.cat(pooled, dim=1)


@pytest.mark.parametrize("act", X.ACTIVATIONS)
def test_cin_matches_triple_loop(act):
    case = ("tiny", 3, 4, (5, 17, 1), 3)
    rows, Ws, bs, _, _ = X.op_inputs(case)
    x0 = rows[:, :12].reshape(3, 3, 4).double()
    Ws, bs = [w.double() for w in Ws], [b.double() for b in bs]
    got = X.cin(x0, Ws, bs, act)
    want = loop_cin(x0, Ws, bs, act)
    assert got.shape == (3, 23)
    torch.testing.assert_close(got, want, atol=1e-12, rtol=1e-12)
    if act == "relu":  # the activation bites: some maps are clipped, and not all
        ident = X.cin(x0, Ws, bs, "identity")
        assert not torch.equal(got, ident)


def test_cin_accepts_conv1d_weights_and_chunks():
    case = ("tiny", 3, 4, (5, 17, 1), 7)
    rows, Ws, bs, _, _ = X.op_inputs(case)
    x0 = rows[:, :12].reshape(7, 3, 4).double()
    Ws, bs = [w.double() for w in Ws], [b.double() for b in bs]
    whole = X.cin(x0, Ws, bs, "relu")
    torch.testing.assert_close(X.cin(x0, [w.unsqueeze(2) for w in Ws], bs, "relu", chunk=3), whole, atol=0, rtol=0)


def small_model(act="identity", **kw):
    torch.manual_seed(42)
    m = rankops.XDeepFM(None, cin_activation=act, vocab_sizes=SMALL, **kw)
    return H.randomize_eval_stats(m, 43).eval()


def test_creation_order_and_keys():
    m = small_model(cin_layer_sizes=(5, 17, 1))
    assert [n for n, _ in m.named_children()] == [
        "first_order_embeddings", "second_order_embeddings", "deep_layers", "deep_output_layer", "final_layer",
        "cin_layers", "cin_output_layer"]
    f = m.num_categories
    assert f == 6 and list(m.second_order_embeddings) == list(rankops.deepfm.WECHAT_FIELDS)
    assert [tuple(c.weight.shape) for c in m.cin_layers] == [(5, f * f, 1), (17, 5 * f, 1), (1, 17 * f, 1)]
    assert all(isinstance(c, torch.nn.Conv1d) and c.bias is not None for c in m.cin_layers)
    assert tuple(m.cin_output_layer.weight.shape) == (1, 23)
    assert tuple(m.final_layer.weight.shape) == (1, 3)
    d = rankops.DeepFM(None, vocab_sizes=SMALL)
    dk, xk = list(d.state_dict()), list(m.state_dict())
    assert xk[:len(dk)] == dk  # DeepFM's keys first, in DeepFM's order
    assert all(k.startswith(("cin_layers.", "cin_output_layer.")) for k in xk[len(dk):])
    res = m.load_state_dict(d.state_dict(), strict=False)
    assert not res.unexpected_keys and all(k.startswith(("cin_layers.", "cin_output_layer.")) for k in res.missing_keys)
    default = rankops.XDeepFM(None, vocab_sizes=SMALL)
    assert default.cin_layer_sizes == (128, 128) and default.cin_activation == "identity"
    assert [l.linear.out_features for l in default._tail] == [512, 256, 128]
    with pytest.raises(ValueError):
        rankops.XDeepFM(None, vocab_sizes=SMALL, cin_activation="tanh")


def test_same_seed_same_shared_parameters_as_deepfm():
    torch.manual_seed(5)
    d = rankops.DeepFM(None, vocab_sizes=SMALL)
    torch.manual_seed(5)
    x = rankops.XDeepFM(None, vocab_sizes=SMALL)
    xs = x.state_dict()
    for k, v in d.state_dict().items():
        assert torch.equal(v, xs[k]), k
    fields = {f"f{i}": 11 + i for i in range(5)}
    torch.manual_seed(6)
    d = rankops.DeepFM(None, embedding_dim=4, hidden_units=[32, 8], batch_norm=False, vocab_sizes=fields)
    torch.manual_seed(6)
    x = rankops.XDeepFM(None, embedding_dim=4, hidden_units=[32, 8], batch_norm=False, vocab_sizes=fields)
    for k, v in d.state_dict().items():
        assert torch.equal(v, x.state_dict()[k]), k


@pytest.mark.parametrize("batch_norm", [True, False])
def test_linear_and_deep_parts_are_the_oracles_deepfm(batch_norm):
    m = small_model(batch_norm=batch_norm)
    p = X.floats(H.cpu_params(m), torch.float64)
    cat = H.deepfm_inputs(33, SMALL, 9)["category"]
    prob, total, linear, cin_logit, deep = X.forward(p, cat)
    _, _, fm1, _, deep_ref = ref.deepfm_forward(p, cat, list(rankops.deepfm.WECHAT_FIELDS), 3, batch_norm)
    torch.testing.assert_close(linear, fm1, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(deep, deep_ref, atol=1e-12, rtol=1e-12)
    for t in (prob, total, linear, cin_logit, deep):
        assert t.shape == (33, 1) and t.dtype == torch.float64
    want = torch.cat([linear, cin_logit, deep], 1) @ p["final_layer.weight"].t() + p["final_layer.bias"]
    torch.testing.assert_close(total, want, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(prob, torch.sigmoid(total), atol=0, rtol=0)


def test_train_mode_and_cpu_tensors_raise():
    m = small_model()
    cat = H.deepfm_inputs(4, SMALL, 9)["category"]
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m(cat)
    m.train()
    with pytest.raises(NotImplementedError):
        m(cat)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        m(cat)


def measured_drifts():
    """float32 against float64 of the restatement at the GPU tests' seeded inputs."""
    pooled = logit = prob = 0.0
    for case in X.OP_CASES:
        for act in X.ACTIVATIONS:
            p64, l64 = X.op_reference(case, act, torch.float64)
            p32, l32 = X.op_reference(case, act, torch.float32)
            pooled = max(pooled, X.rel_err(p32, p64))
            logit = max(logit, X.rel_err(l32, l64))
    for case in X.MODEL_CASES:
        model = X.build_model(case)
        p = H.cpu_params(model)
        cat = X.model_inputs(case)
        o64 = X.forward(X.floats(p, torch.float64), cat)
        o32 = X.forward(X.floats(p, torch.float32), cat)
        prob = max(prob, X.rel_err(o32[0], o64[0]))
        logit = max(logit, max(X.rel_err(a, b) for a, b in zip(o32[1:], o64[1:])))
    return pooled, logit, prob


def test_tolerances_are_50x_the_measured_fp32_drift():
    pooled, logit, prob = measured_drifts()
    print(f"fp32 drift: pooled {pooled:.3g}  logit {logit:.3g}  probability {prob:.3g}")
    for name, tol, drift in (("POOLED_TOL", X.POOLED_TOL, pooled), ("LOGIT_TOL", X.LOGIT_TOL, logit),
                             ("PROB_TOL", X.PROB_TOL, prob)):
        assert 25 * drift <= tol <= 100 * drift, (name, tol, drift)
