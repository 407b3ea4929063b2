"""CPU tests of the MMoE restatement (tests/mmoe_ref.py) the GPU tests compare against: it is tied to an
independent per-row loop and, stack by stack, to the oracle's DCN dnn; the module's creation order and
keys are the definition's; the tolerance constants are 50 x the float32 drift measured here; and the
seeded cases are such that a wrong mix, gate or ReLU could not hide."""
import math

import pytest
import torch

import helpers as H
import mmoe_ref as R
import rankops
from oracle import reference_forward as ref

ORDINARY = [c for c in R.OP_CASES if c[0] != R.EXTREME]


def loop_mmoe(x, experts, gates, towers):
    """The definition read row by row with Python floats: every dot product its own sum."""
    def lin(v, W, b):
        return [sum(float(W[n, j]) * v[j] for j in range(W.shape[1])) + (float(b[n]) if b is not None else 0.0)
                for n in range(W.shape[0])]

    def run(v, layers):
        for W, b in layers:
            v = [max(z, 0.0) for z in lin(v, W, b)]
        return v
    mixed, gate_probs, logits = [], [], []
    for row in x:
        v = [float(t) for t in row]
        f = [run(v, layers) for layers in experts]
        mrow, grow, lrow = [], [], []
        for (Wg, bg), (hidden, (w_out, b_out)) in zip(gates, towers):
            z = lin(v, Wg, bg)
            top = max(z)
            ex = [math.exp(t - top) for t in z]
            g = [t / sum(ex) for t in ex]
            m = [sum(g[e] * f[e][h] for e in range(len(f))) for h in range(len(f[0]))]
            t = run(m, hidden)
            lrow.append(sum(float(w_out.reshape(-1)[j]) * t[j] for j in range(len(t))) + float(b_out))
            mrow.append(m)
            grow.append(g)
        mixed.append(mrow)
        gate_probs.append(grow)
        logits.append(lrow)
    logits = torch.tensor(logits, dtype=torch.float64)
    return (torch.tensor(mixed, dtype=torch.float64), torch.tensor(gate_probs, dtype=torch.float64), logits,
            1 / (1 + torch.exp(-logits)))


def test_restatement_matches_per_row_loop():
    c = ("tiny", 11, 3, 2, (9, 5), (4,), 5)
    rows, experts, gates, towers = R.op_inputs(c)
    x = rows[:, :11].double()
    experts, gates, towers = R.cast(experts, torch.float64), R.cast(gates, torch.float64), R.cast(towers, torch.float64)
    got = R.mmoe(x, experts, gates, towers)
    want = loop_mmoe(x, experts, gates, towers)
    assert [tuple(t.shape) for t in got] == [(5, 2, 5), (5, 2, 3), (5, 2), (5, 2)]
    for g, w in zip(got, want):
        torch.testing.assert_close(g, w, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(got[1].sum(dim=2), torch.ones(5, 2, dtype=torch.float64), atol=1e-12, rtol=0)
    two = R.mmoe(x, experts, gates)  # without towers: the two tensors only
    assert len(two) == 2 and torch.equal(two[0], got[0]) and torch.equal(two[1], got[1])
    ordered = R.mmoe(x, experts, gates, towers, ordered=True)  # the fixed-order form is the same function
    for g, w in zip(ordered, got):
        torch.testing.assert_close(g, w, atol=1e-12, rtol=1e-12)
    nob = R.mmoe(x, [[(W, None) for W, _ in l] for l in experts], [(W, None) for W, _ in gates])
    zb = R.mmoe(x, [[(W, torch.zeros_like(b)) for W, b in l] for l in experts],
                [(W, torch.zeros_like(b)) for W, b in gates])
    assert torch.equal(nob[0], zb[0]) and torch.equal(nob[1], zb[1])


def oracle_stack(x, layers):
    """Linear + ReLU layers through the oracle's DCN forward: the rows as its dense block (one zero-wide
    table, no cross layer), the stack as its dnn, and output_layer picking one dnn column at a time."""
    B, width = x.shape
    p = {"embeddings.userid.weight": torch.zeros(1, 0, dtype=x.dtype)}
    for i, (W, b) in enumerate(layers):
        p[f"dnn.{2 * i}.weight"], p[f"dnn.{2 * i}.bias"] = W, b
    n = layers[-1][0].shape[0]
    cols = []
    for j in range(n):
        w = torch.zeros(1, width + n, dtype=x.dtype)
        w[0, width + j] = 1
        p["output_layer.weight"], p["output_layer.bias"] = w, torch.zeros(1, dtype=x.dtype)
        _, logit = ref.dcn_forward(p, x, {"userid": torch.zeros(B, dtype=torch.long)}, 0, len(layers), cross=[])
        cols.append(logit)
    return torch.cat(cols, dim=1)


def test_experts_and_towers_are_the_oracles_dnn_stack():
    c = ("tiny", 13, 3, 2, (10, 6), (5, 3), 9)
    rows, experts, gates, towers = R.op_inputs(c)
    x = rows[:, :13].double()
    experts, gates, towers = R.cast(experts, torch.float64), R.cast(gates, torch.float64), R.cast(towers, torch.float64)
    mixed, gate_probs, logits, _ = R.mmoe(x, experts, gates, towers)
    f = torch.stack([oracle_stack(x, layers) for layers in experts], dim=1)
    for e, layers in enumerate(experts):
        torch.testing.assert_close(R.stack(x, layers), f[:, e], atol=1e-12, rtol=1e-12)
    want = torch.einsum("bke,beh->bkh", gate_probs, f)
    torch.testing.assert_close(mixed, want, atol=1e-12, rtol=1e-12)
    for k, (hidden, (w_out, b_out)) in enumerate(towers):
        t = oracle_stack(mixed[:, k], hidden)
        torch.testing.assert_close(logits[:, k:k + 1], t @ w_out.t() + b_out, atol=1e-12, rtol=1e-12)


def small_model(**kw):
    torch.manual_seed(42)
    return rankops.MMoE(None, vocab_sizes=H.SMALL_VOCAB, **kw).eval()


def test_creation_order_keys_and_defaults():
    m = small_model()
    assert [n for n, _ in m.named_children()] == ["embeddings", "experts", "gates", "towers", "tower_outputs"]
    assert m.num_experts == 4 and m.task_names == ("read_comment", "like", "click_avatar")
    assert m.expert_hidden_units == (256, 128) and m.tower_hidden_units == (64,) and m.input_dim == 50
    assert len(m.experts) == 4 and len(m.gates) == len(m.towers) == len(m.tower_outputs) == 3
    for seq in m.experts:
        assert [type(l).__name__ for l in seq] == ["Linear", "ReLU", "Dropout", "Linear", "ReLU", "Dropout"]
        assert [tuple(l.weight.shape) for l in seq if isinstance(l, torch.nn.Linear)] == [(256, 50), (128, 256)]
        assert all(l.p == 0.1 for l in seq if isinstance(l, torch.nn.Dropout))
    assert all(tuple(g.weight.shape) == (4, 50) and g.bias is not None for g in m.gates)
    assert all(tuple(t[0].weight.shape) == (64, 128) for t in m.towers)
    assert all(tuple(o.weight.shape) == (1, 64) for o in m.tower_outputs)
    keys = list(m.state_dict())
    want = [f"embeddings.{f}.weight" for f in H.DCN_FIELDS]
    want += [f"experts.{e}.{i}.{s}" for e in range(4) for i in (0, 3) for s in ("weight", "bias")]
    want += [f"gates.{k}.{s}" for k in range(3) for s in ("weight", "bias")]
    want += [f"towers.{k}.0.{s}" for k in range(3) for s in ("weight", "bias")]
    want += [f"tower_outputs.{k}.{s}" for k in range(3) for s in ("weight", "bias")]
    assert keys == want
    nodrop = small_model(dropout_rate=0, tower_hidden_units=(), expert_hidden_units=(24,), num_experts=3,
                         task_names=("a", "b"))
    assert [type(l).__name__ for l in nodrop.experts[0]] == ["Linear", "ReLU"]
    assert all(len(t) == 0 for t in nodrop.towers) and tuple(nodrop.tower_outputs[1].weight.shape) == (1, 24)
    assert R.model_parts(H.cpu_params(nodrop))[2][0][0] == []
    assert rankops.mmoe.MMoE is rankops.MMoE and callable(rankops.mmoe)


def test_same_seed_same_embeddings_as_dcn_and_dcn_checkpoint_loads():
    torch.manual_seed(5)
    d = rankops.DCNModel(None, vocab_sizes=H.SMALL_VOCAB)
    torch.manual_seed(5)
    m = rankops.MMoE(None, vocab_sizes=H.SMALL_VOCAB)
    ms = m.state_dict()
    emb = {k: v for k, v in d.state_dict().items() if k.startswith("embeddings.")}
    assert list(emb) == [k for k in ms if k.startswith("embeddings.")]
    for k, v in emb.items():
        assert torch.equal(v, ms[k]), k
    other = small_model()
    res = other.load_state_dict(emb, strict=False)
    assert not res.unexpected_keys and not any(k.startswith("embeddings.") for k in res.missing_keys)
    assert m.vocab_sizes == d.vocab_sizes


def test_constructor_errors():
    for kw in (dict(num_experts=0), dict(expert_hidden_units=()), dict(expert_hidden_units=(16, 0)),
               dict(tower_hidden_units=(-1,)), dict(task_names=()), dict(task_names=("a", "a")),
               dict(dropout_rate=1.0)):
        with pytest.raises(ValueError):
            rankops.MMoE(None, vocab_sizes=H.SMALL_VOCAB, **kw)


def test_train_mode_and_cpu_tensors_raise():
    m = small_model()
    inp = H.dcn_inputs(4, H.SMALL_VOCAB)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m(inp["dense"], inp["category"])
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rankops.mmoe(torch.zeros(2, 8), [[(torch.zeros(4, 8), None)]], [(torch.zeros(1, 8), None)])
    m.train()
    with pytest.raises(NotImplementedError):
        m(inp["dense"], inp["category"])
    with torch.no_grad(), pytest.raises(NotImplementedError):
        m(inp["dense"], inp["category"])
    with pytest.raises(RuntimeError, match="eval mode"):
        m.prepare(inp["dense"], inp["category"])


def test_mmoe_fits_mirrors_the_envelope():
    fits = rankops.common.mmoe_fits
    assert fits(50, 7, 4, 3, (256, 128), (64,)) and fits(200, 1, 16, 4, (512,), (512,))
    assert fits(256, 16, 16, 4, (512, 512, 512), (512, 512, 512)) and fits(50, 7, 8, 8, (16,), ())
    assert not fits(257, 1, 4, 3, (16,), ()) and not fits(50, 17, 4, 3, (16,), ())
    assert not fits(50, 1, 17, 1, (16,), ()) and not fits(50, 1, 4, 9, (16,), ()) and not fits(50, 1, 13, 5, (16,), ())
    assert not fits(50, 1, 4, 3, (513,), ()) and not fits(50, 1, 4, 3, (16,), (513,))
    assert not fits(50, 1, 4, 3, (), ()) and not fits(50, 1, 4, 3, (8, 8, 8, 8), ())
    assert not fits(50, 1, 4, 3, (8,), (8,) * 4)


def measured_drifts():
    """float32 against float64 of the restatement at the GPU tests' seeded inputs:
    ([mixed, gates, logits, probs] of the ordinary cases and the model cases, the same of extreme_gate).
    The float32 run takes every sum in a fixed order (mmoe_ref.linear), so the figures do not depend on
    the machine's matmul."""
    def over(cases):
        d = [0.0] * 4
        for c in cases:
            o64, o32 = R.op_reference(c, torch.float64), R.op_reference(c, torch.float32, ordered=True)
            d = [max(a, R.rel_err(x, y)) for a, x, y in zip(d, o32, o64)]
        return d
    ordinary, extreme = over(ORDINARY), over([R.case(R.EXTREME)])
    for mc in R.MODEL_CASES:
        p = H.cpu_params(R.build_model(mc))
        inp = R.model_inputs(mc)
        prob64, logit64 = R.forward(R.floats(p, torch.float64), inp["dense"], inp["category"])
        prob32, logit32 = R.forward(R.floats(p, torch.float32), inp["dense"], inp["category"], ordered=True)
        ordinary[2] = max(ordinary[2], R.rel_err(logit32, logit64))
        ordinary[3] = max(ordinary[3], R.rel_err(prob32, prob64))
    return ordinary, extreme


def test_tolerances_are_50x_the_measured_fp32_drift():
    ordinary, extreme = measured_drifts()
    names = ("MIXED_TOL", "GATE_TOL", "LOGIT_TOL", "PROB_TOL")
    print("fp32 drift, ordinary:", "  ".join(f"{n} {d:.3g}" for n, d in zip(names, ordinary)))
    print("fp32 drift, extreme_gate:", "  ".join(f"{n} {d:.3g}" for n, d in zip(names, extreme)))
    for n, tol, drift in zip(names, R.tolerances("wechat"), ordinary):
        assert 25 * drift <= tol <= 100 * drift, (n, tol, drift)
    for n, tol, drift in zip(names, R.tolerances(R.EXTREME), extreme):
        assert 25 * drift <= tol <= 100 * drift, ("EXTREME_" + n, tol, drift)


@pytest.mark.parametrize("c", R.OP_CASES, ids=[c[0] for c in R.OP_CASES])
def test_cases_cannot_hide_a_failure(c):
    """On the float64 reference alone: the gates are neither uniform nor one-hot (a wrong mix would show),
    extreme_gate is near one-hot, and every ReLU clips a fair share (and not all) of its inputs."""
    name, width, E, K, eu, tu, B = c
    clipped = []
    mixed, gates, logits, probs = R.op_reference(c, torch.float64, clipped)
    assert mixed.shape == (B, K, eu[-1]) and gates.shape == (B, K, E) and logits.shape == probs.shape == (B, K)
    assert len(clipped) == E * len(eu) + K * len(tu)
    assert all(0.2 <= s <= 0.8 for s in clipped), clipped
    top = gates.max(dim=2).values
    mean_top, near_one_hot = float(top.mean()), float((top > 0.95).double().mean())
    print(f"{name}: largest gate mean {mean_top:.3f}, share above 0.95 {near_one_hot:.3f}, "
          f"ReLU clip shares {min(clipped):.2f}-{max(clipped):.2f}")
    if name == R.EXTREME:
        assert near_one_hot > 0.9
        assert all(bool(torch.isfinite(t).all()) for t in (mixed, gates, logits, probs))
    elif E > 1:
        assert 1.5 / E <= mean_top <= 0.85
        assert near_one_hot <= 0.15
    else:  # one expert: the gate is 1 and the mixture is the expert's output
        rows, experts, _, _ = R.op_inputs(c)
        assert torch.equal(gates, torch.ones_like(gates))
        torch.testing.assert_close(mixed[:, 0], R.stack(rows[:, :width].double(), R.cast(experts[0], torch.float64)),
                                   atol=1e-15, rtol=0)
