"""CPU tests of the FiBiNET restatement (tests/fibinet_ref.py) the GPU tests compare against: it is tied
to a literal loop over (b, pair, d) of the definition and to the oracle's DeepFM, the module's creation
order and keys are the definition's, the seeded SENET inputs clip some attention values and not all, and
the tolerance constants are 50 x the float32 drift measured here."""
import pytest
import torch

import fibinet_ref as X
import helpers as H
import rankops
from oracle import reference_forward as ref

SMALL = {f: H.SMALL_VOCAB[f] for f in rankops.deepfm.WECHAT_FIELDS}  # the six wechat fields


def loop_interaction(x0, w1, w2, We, Wv, bilinear_type):
    """The definition read literally: every c[b, p, d] by its own sums."""
    B, m, D = x0.shape
    r = w1.shape[0]
    P = m * (m - 1) // 2
    c = torch.zeros(B, 2 * P * D, dtype=x0.dtype)
    a = torch.zeros(B, m, dtype=x0.dtype)
    for b in range(B):
        z = [sum(float(x0[b, i, d]) for d in range(D)) / D for i in range(m)]
        h = [max(0.0, sum(float(w1[k, i]) * z[i] for i in range(m))) for k in range(r)]
        for i in range(m):
            a[b, i] = max(0.0, sum(float(w2[i, k]) * h[k] for k in range(r)))
        p = 0
        for i in range(m):
            for j in range(i + 1, m):
                n = {"all": 0, "each": i, "interaction": p}[bilinear_type]
                for d in range(D):
                    pe = sum(float(We[n][d, k]) * float(x0[b, i, k]) for k in range(D))
                    pv = sum(float(Wv[n][d, k]) * float(a[b, i]) * float(x0[b, i, k]) for k in range(D))
                    c[b, p * D + d] = pe * float(x0[b, j, d])
                    c[b, (P + p) * D + d] = pv * float(a[b, j]) * float(x0[b, j, d])
                p += 1
    return c, a


@pytest.mark.parametrize("bilinear_type", X.BILINEAR_TYPES)
def test_interaction_matches_literal_loop(bilinear_type):
    case = ("tiny", 3, 4, 3)
    rows, w1, w2, We, Wv = X.op_inputs(case, bilinear_type, seed=8)  # (a seed that leaves live attention values)
    x0 = rows[:, :12].reshape(3, 3, 4).double()
    w1, w2, We, Wv = w1.double(), w2.double(), [w.double() for w in We], [w.double() for w in Wv]
    assert len(We) == len(Wv) == {"all": 1, "each": 2, "interaction": 3}[bilinear_type]
    c, a = X.interaction(x0, w1, w2, We, Wv, bilinear_type)
    want_c, want_a = loop_interaction(x0, w1, w2, We, Wv, bilinear_type)
    assert c.shape == (3, 3 * 2 * 4) and a.shape == (3, 3)
    torch.testing.assert_close(c, want_c, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(a, want_a, atol=1e-12, rtol=1e-12)
    assert bool((a > 0).any()) and bool((c[:, 12:] != 0).any())  # the q block is not all zeros here
    # column order: all of p (pairs (0,1), (0,2), (1,2)), then all of q
    n = {"all": [0, 0, 0], "each": [0, 0, 1], "interaction": [0, 1, 2]}[bilinear_type]
    for p, (i, j) in enumerate([(0, 1), (0, 2), (1, 2)]):
        torch.testing.assert_close(c[:, 4 * p:4 * p + 4], (x0[:, i] @ We[n[p]].t()) * x0[:, j], atol=1e-12, rtol=1e-12)
        v = a.unsqueeze(2) * x0
        torch.testing.assert_close(c[:, 12 + 4 * p:16 + 4 * p], (v[:, i] @ Wv[n[p]].t()) * v[:, j], atol=1e-12,
                                   rtol=1e-12)


def small_model(**kw):
    torch.manual_seed(42)
    m = rankops.FiBiNET(None, vocab_sizes=SMALL, **kw)
    return H.randomize_eval_stats(m, 43).eval()


@pytest.mark.parametrize("bilinear_type", X.BILINEAR_TYPES)
def test_creation_order_and_keys(bilinear_type):
    m = small_model(bilinear_type=bilinear_type)
    assert [n for n, _ in m.named_children()] == [
        "first_order_embeddings", "second_order_embeddings", "senet", "bilinear_embedding", "bilinear_senet",
        "deep_layers", "deep_output_layer", "final_layer"]
    f, D = m.num_categories, m.embedding_dim
    assert f == 6 and D == 8 and list(m.second_order_embeddings) == list(rankops.deepfm.WECHAT_FIELDS)
    n = {"all": 1, "each": f - 1, "interaction": f * (f - 1) // 2}[bilinear_type]
    assert len(m.bilinear_embedding) == len(m.bilinear_senet) == n
    for l in list(m.bilinear_embedding) + list(m.bilinear_senet):
        assert isinstance(l, torch.nn.Linear) and tuple(l.weight.shape) == (D, D) and l.bias is None
    keys = list(m.state_dict())
    assert [k for k in keys if k.startswith("senet.")] == ["senet.0.weight", "senet.2.weight"]
    assert tuple(m.senet[0].weight.shape) == (2, 6) and tuple(m.senet[2].weight.shape) == (6, 2)  # r = 6 // 3
    assert tuple(m.final_layer.weight.shape) == (1, 2)
    assert m.deep_layers[0].in_features == f * (f - 1) * D
    assert [l.linear.out_features for l in m._tail] == [512, 256, 128]
    order = [k.split(".")[0] for k in keys]
    assert sorted(set(order), key=order.index) == [
        "first_order_embeddings", "second_order_embeddings", "senet", "bilinear_embedding", "bilinear_senet",
        "deep_layers", "deep_output_layer", "final_layer"]


def test_reduction_ratio_and_errors():
    assert small_model(reduction_ratio=1).reduced == 6
    assert small_model(reduction_ratio=7).reduced == 1  # r = max(1, m // ratio)
    with pytest.raises(ValueError):
        rankops.FiBiNET(None, vocab_sizes=SMALL, bilinear_type="field")
    with pytest.raises(ValueError):
        rankops.FiBiNET(None, vocab_sizes=SMALL, reduction_ratio=0)
    m = small_model()
    cat = H.deepfm_inputs(4, SMALL, 9)["category"]
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m(cat)
    m.train()
    with pytest.raises(NotImplementedError):
        m(cat)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        m(cat)


def test_same_seed_gives_deepfms_tables_and_its_keys_load():
    torch.manual_seed(5)
    d = rankops.DeepFM(None, vocab_sizes=SMALL)
    torch.manual_seed(5)
    x = rankops.FiBiNET(None, vocab_sizes=SMALL)
    xs, ds = x.state_dict(), d.state_dict()
    tables = [k for k in ds if k.startswith(("first_order_embeddings.", "second_order_embeddings."))]
    assert len(tables) == 12 and list(xs)[:12] == tables  # DeepFM's names and order
    for k in tables:
        assert torch.equal(ds[k], xs[k]), k
    torch.manual_seed(6)
    other = rankops.DeepFM(None, vocab_sizes=SMALL)
    res = x.load_state_dict({k: v for k, v in other.state_dict().items() if k in tables}, strict=False)
    assert not res.unexpected_keys and not any(k in tables for k in res.missing_keys)
    for k in tables:
        assert torch.equal(x.state_dict()[k], other.state_dict()[k]), k


@pytest.mark.parametrize("batch_norm", [True, False])
def test_linear_and_head_are_consistent_with_the_oracle(batch_norm):
    m = small_model(batch_norm=batch_norm)
    p = X.floats(H.cpu_params(m), torch.float64)
    cat = H.deepfm_inputs(33, SMALL, 9)["category"]
    prob, total, linear, deep = X.forward(p, cat)
    torch.manual_seed(42)
    d = rankops.DeepFM(None, vocab_sizes=SMALL, batch_norm=batch_norm)  # the same seed: the same tables
    dp = X.floats(H.cpu_params(H.randomize_eval_stats(d, 43).eval()), torch.float64)
    _, _, fm1, _, _ = ref.deepfm_forward(dp, cat, list(rankops.deepfm.WECHAT_FIELDS), 3, batch_norm)
    torch.testing.assert_close(linear, fm1, atol=1e-12, rtol=1e-12)
    for t in (prob, total, linear, deep):
        assert t.shape == (33, 1) and t.dtype == torch.float64
    want = torch.cat([linear, deep], 1) @ p["final_layer.weight"].t() + p["final_layer.bias"]
    torch.testing.assert_close(total, want, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(prob, torch.sigmoid(total), atol=0, rtol=0)
    assert X.bilinear_type_of(p) == "interaction"


@pytest.mark.parametrize("case", X.OP_CASES, ids=[c[0] for c in X.OP_CASES])
def test_senet_relus_bite_and_not_everywhere(case):
    _, a = X.op_reference(case, "all")
    share = float((a == 0).double().mean())
    print(f"{case[0]}: share of zero attention values {share:.3f}")
    assert 0.2 <= share <= 0.8


def measured_drifts():
    """float32 against float64 of the restatement at the GPU tests' seeded inputs."""
    c = attn = logit = prob = 0.0
    for case in X.OP_CASES:
        for t in X.BILINEAR_TYPES:
            c64, a64 = X.op_reference(case, t, torch.float64)
            c32, a32 = X.op_reference(case, t, torch.float32)
            c, attn = max(c, X.rel_err(c32, c64)), max(attn, X.rel_err(a32, a64))
    for case in X.MODEL_CASES:
        p = H.cpu_params(X.build_model(case))
        cat = X.model_inputs(case)
        o64 = X.forward(X.floats(p, torch.float64), cat)
        o32 = X.forward(X.floats(p, torch.float32), cat)
        prob = max(prob, X.rel_err(o32[0], o64[0]))
        logit = max(logit, max(X.rel_err(a, b) for a, b in zip(o32[1:], o64[1:])))
    return c, attn, logit, prob


def test_tolerances_are_50x_the_measured_fp32_drift():
    c, attn, logit, prob = measured_drifts()
    print(f"fp32 drift: c {c:.3g}  attention {attn:.3g}  logit {logit:.3g}  probability {prob:.3g}")
    for name, tol, drift in (("C_TOL", X.C_TOL, c), ("ATTN_TOL", X.ATTN_TOL, attn), ("LOGIT_TOL", X.LOGIT_TOL, logit),
                             ("PROB_TOL", X.PROB_TOL, prob)):
        assert 25 * drift <= tol <= 100 * drift, (name, tol, drift)
