"""CPU tests of the PLE restatement (tests/ple_ref.py) the GPU tests compare against: it is tied to an
independent per-row loop and, at L = 1 and ms = 0, to the MMoE restatement; the module's creation order and
keys are the definition's; the tolerance constants are 50 x the float32 drift measured here; and the seeded
cases are such that a wrong mix, gate, input or ReLU could not hide."""
import math

import pytest
import torch

import helpers as H
import mmoe_ref
import ple_ref as R
import rankops

ORDINARY = [c for c in R.OP_CASES if c[0] != R.EXTREME]
CASE_IDS = [c[0] for c in R.OP_CASES]


def loop_ple(x, levels, towers):
    """The definition read row by row with Python floats: every dot product its own sum."""
    def lin(v, W, b):
        return [sum(float(W[n, j]) * v[j] for j in range(W.shape[1])) + (float(b[n]) if b is not None else 0.0)
                for n in range(W.shape[0])]

    def run(v, layers):
        for W, b in layers:
            v = [max(z, 0.0) for z in lin(v, W, b)]
        return v

    def softmax(z):
        top = max(z)
        ex = [math.exp(t - top) for t in z]
        return [t / sum(ex) for t in ex]

    def blend(g, fs):
        return [sum(g[c] * fs[c][h] for c in range(len(fs))) for h in range(len(fs[0]))]
    K = len(levels[0][2])
    per_level = [([], [], []) for _ in levels]
    logits = []
    for row in x:
        xk, xs = [[float(t) for t in row]] * K, [float(t) for t in row]
        for j, (specific, shared, gates, shared_gate) in enumerate(levels):
            fk = [[run(xk[k], layers) for layers in specific[k]] for k in range(K)]
            fs = [run(xs, layers) for layers in shared]
            gk = [softmax(lin(xk[k], *gates[k])) for k in range(K)]
            new = [blend(gk[k], fk[k] + fs) for k in range(K)]
            reps = list(new)
            if shared_gate is not None:
                gsh = softmax(lin(xs, *shared_gate))
                xs = blend(gsh, [f for task in fk for f in task] + fs)
                reps.append(xs)
                per_level[j][2].append(gsh)
            xk = new
            per_level[j][0].append(reps)
            per_level[j][1].append(gk)
        lrow = []
        for k, (hidden, (w_out, b_out)) in enumerate(towers):
            t = run(xk[k], hidden)
            lrow.append(sum(float(w_out.reshape(-1)[i]) * t[i] for i in range(len(t))) + float(b_out))
        logits.append(lrow)
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731
    logits = f64(logits)
    return ([(f64(r), f64(g), f64(s) if s else None) for r, g, s in per_level], logits, 1 / (1 + torch.exp(-logits)))


def assert_same(got, want, tol=1e-12):
    for a, b in zip(R.flat(got), R.flat(want)):
        assert len(a) == len(b)
        for s, t in zip(a, b):
            torch.testing.assert_close(s, t, atol=tol, rtol=tol)


def test_restatement_matches_per_row_loop():
    c = ("tiny", 11, 3, 2, 2, 1, (9, 5), (4,), 5)
    rows, levels, towers = R.op_inputs(c)
    x = rows[:, :11].double()
    levels, towers = R.cast(levels, torch.float64), R.cast(towers, torch.float64)
    got = R.ple(x, levels, towers)
    want = loop_ple(x, levels, towers)
    assert [tuple(lv[0].shape) for lv in got[0]] == [(5, 3, 5), (5, 3, 5), (5, 2, 5)]
    assert [tuple(lv[1].shape) for lv in got[0]] == [(5, 2, 3)] * 3
    assert [None if lv[2] is None else tuple(lv[2].shape) for lv in got[0]] == [(5, 5), (5, 5), None]
    assert got[1].shape == got[2].shape == (5, 2)
    assert_same(got, want)
    for reps, gk, gs in got[0]:
        torch.testing.assert_close(gk.sum(dim=2), torch.ones(5, 2, dtype=torch.float64), atol=1e-12, rtol=0)
        if gs is not None:
            torch.testing.assert_close(gs.sum(dim=1), torch.ones(5, dtype=torch.float64), atol=1e-12, rtol=0)
    bare = R.ple(x, levels)  # without towers: the levels only
    assert bare[1] is None and bare[2] is None
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(bare[0], got[0]))
    assert_same(R.ple(x, levels, towers, ordered=True), got)  # the fixed-order form is the same function

    def biases(f):
        return [([[[(W, f(b)) for W, b in e] for e in task] for task in sp], [[(W, f(b)) for W, b in e] for e in sh],
                 [(W, f(b)) for W, b in gt], None if sg is None else (sg[0], f(sg[1]))) for sp, sh, gt, sg in levels]
    assert_same(R.ple(x, biases(lambda b: None), towers), R.ple(x, biases(torch.zeros_like), towers), 0)


def test_one_level_without_task_experts_is_mmoe():
    c = mmoe_ref.case("deep")
    rows, experts, gates, towers = mmoe_ref.op_inputs(c)
    x = rows[:, :c[1]].double()
    experts, gates, towers = (R.cast(t, torch.float64) for t in (experts, gates, towers))
    mixed, gate_probs, logits, probs = mmoe_ref.mmoe(x, experts, gates, towers)
    levels, plogits, pprobs = R.ple(x, [([[] for _ in gates], experts, gates, None)], towers)
    assert len(levels) == 1 and levels[0][2] is None
    assert torch.equal(levels[0][0], mixed) and torch.equal(levels[0][1], gate_probs)
    assert torch.equal(plogits, logits) and torch.equal(pprobs, probs)
    for a, b in zip(R.ple(x.float(), [([[] for _ in gates], R.cast(experts, torch.float32), R.cast(gates, torch.float32),
                                      None)], R.cast(towers, torch.float32), ordered=True)[1:],
                    mmoe_ref.mmoe(x.float(), R.cast(experts, torch.float32), R.cast(gates, torch.float32),
                                  R.cast(towers, torch.float32), ordered=True)[2:]):
        assert torch.equal(a, b)


def small_model(**kw):
    torch.manual_seed(42)
    return rankops.PLE(None, vocab_sizes=H.SMALL_VOCAB, **kw).eval()


def test_creation_order_keys_and_defaults():
    m = small_model()
    assert [n for n, _ in m.named_children()] == ["embeddings", "levels", "towers", "tower_outputs"]
    assert (m.num_levels, m.num_specific_experts, m.num_shared_experts) == (2, 2, 2)
    assert m.task_names == ("read_comment", "like", "click_avatar")
    assert m.expert_hidden_units == (256, 128) and m.tower_hidden_units == (64,) and m.input_dim == 50
    assert [[n for n, _ in lv.named_children()] for lv in m.levels] == [
        ["specific_experts", "shared_experts", "gates", "shared_gate"], ["specific_experts", "shared_experts", "gates"]]
    for j, lv in enumerate(m.levels):
        k_in = 50 if j == 0 else 128
        assert len(lv.specific_experts) == 3 and all(len(t) == 2 for t in lv.specific_experts)
        assert len(lv.shared_experts) == 2 and len(lv.gates) == 3
        for seq in lv.stacks():
            assert [type(l).__name__ for l in seq] == ["Linear", "ReLU", "Dropout", "Linear", "ReLU", "Dropout"]
            assert [tuple(l.weight.shape) for l in seq if isinstance(l, torch.nn.Linear)] == [(256, k_in), (128, 256)]
            assert all(l.p == 0.1 for l in seq if isinstance(l, torch.nn.Dropout))
        assert all(tuple(g.weight.shape) == (4, k_in) and g.bias is not None for g in lv.gates)
    assert tuple(m.levels[0].shared_gate.weight.shape) == (8, 50)
    assert all(tuple(t[0].weight.shape) == (64, 128) for t in m.towers)
    assert all(tuple(o.weight.shape) == (1, 64) for o in m.tower_outputs)
    keys = list(m.state_dict())
    want = [f"embeddings.{f}.weight" for f in H.DCN_FIELDS]
    for j in range(2):
        want += [f"levels.{j}.specific_experts.{k}.{i}.{l}.{s}" for k in range(3) for i in range(2) for l in (0, 3)
                 for s in ("weight", "bias")]
        want += [f"levels.{j}.shared_experts.{i}.{l}.{s}" for i in range(2) for l in (0, 3) for s in ("weight", "bias")]
        want += [f"levels.{j}.gates.{k}.{s}" for k in range(3) for s in ("weight", "bias")]
        if j == 0:
            want += [f"levels.0.shared_gate.{s}" for s in ("weight", "bias")]
    want += [f"towers.{k}.0.{s}" for k in range(3) for s in ("weight", "bias")]
    want += [f"tower_outputs.{k}.{s}" for k in range(3) for s in ("weight", "bias")]
    assert keys == want
    nodrop = small_model(dropout_rate=0, tower_hidden_units=(), expert_hidden_units=(24,), num_levels=1,
                         num_specific_experts=0, num_shared_experts=3, task_names=("a", "b"))
    assert [type(l).__name__ for l in nodrop.levels[0].shared_experts[0]] == ["Linear", "ReLU"]
    assert all(len(t) == 0 for t in nodrop.levels[0].specific_experts) and not hasattr(nodrop.levels[0], "shared_gate")
    assert all(len(t) == 0 for t in nodrop.towers) and tuple(nodrop.tower_outputs[1].weight.shape) == (1, 24)
    levels, towers = R.model_parts(H.cpu_params(nodrop))
    assert towers[0][0] == [] and levels[0][0] == [[], []] and len(levels[0][1]) == 3 and levels[0][3] is None
    assert rankops.ple.PLE is rankops.PLE and callable(rankops.ple)


def test_same_seed_same_embeddings_as_dcn_and_dcn_checkpoint_loads():
    torch.manual_seed(5)
    d = rankops.DCNModel(None, vocab_sizes=H.SMALL_VOCAB)
    torch.manual_seed(5)
    m = rankops.PLE(None, vocab_sizes=H.SMALL_VOCAB)
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
    for kw in (dict(num_levels=0), dict(num_specific_experts=-1), dict(num_shared_experts=0),
               dict(expert_hidden_units=()), dict(expert_hidden_units=(16, 0)), dict(tower_hidden_units=(-1,)),
               dict(task_names=()), dict(task_names=("a", "a")), dict(dropout_rate=1.0)):
        with pytest.raises(ValueError):
            rankops.PLE(None, vocab_sizes=H.SMALL_VOCAB, **kw)
    assert rankops.PLE(None, vocab_sizes=H.SMALL_VOCAB, num_specific_experts=0, num_levels=1).fits()


def test_train_mode_and_cpu_tensors_raise():
    m = small_model()
    inp = H.dcn_inputs(4, H.SMALL_VOCAB)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m(inp["dense"], inp["category"])
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rankops.ple(torch.zeros(2, 8), [([[]], [[(torch.zeros(4, 8), None)]], [(torch.zeros(1, 8), None)], None)])
    m.train()
    with pytest.raises(NotImplementedError):
        m(inp["dense"], inp["category"])
    with torch.no_grad(), pytest.raises(NotImplementedError):
        m(inp["dense"], inp["category"])
    with pytest.raises(RuntimeError, match="eval mode"):
        m.prepare(inp["dense"], inp["category"])


def test_ple_fits_mirrors_the_envelope():
    fits = rankops.common.ple_fits  # (width, segments, L, K, ms, mc, expert units, tower units)
    assert fits(50, 7, 2, 3, 2, 2, (256, 128), (64,)) and fits(50, 7, 3, 3, 2, 2, (256, 128), (64,))
    assert fits(50, 7, 4, 2, 1, 1, (16,), ()) and not fits(50, 7, 5, 2, 1, 1, (16,), ()) and not fits(50, 7, 0, 2, 1, 1, (16,), ())
    assert fits(50, 7, 2, 8, 2, 2, (256, 64), (64,)) and not fits(50, 7, 2, 9, 2, 2, (16,), ())
    assert not fits(50, 7, 2, 0, 2, 2, (16,), ())
    assert fits(50, 7, 2, 8, 7, 8, (16,), ()) and not fits(50, 7, 2, 8, 7, 9, (16,), ())       # K ms + mc = 64 | 65
    assert fits(50, 7, 1, 3, 0, 64, (16,), ()) and not fits(50, 7, 1, 3, 0, 65, (16,), ())
    assert fits(50, 7, 2, 3, 0, 1, (16,), ()) and not fits(50, 7, 2, 3, -1, 2, (16,), ()) and not fits(50, 7, 2, 3, 2, 0, (16,), ())
    assert fits(256, 16, 2, 2, 1, 1, (16,), ()) and not fits(257, 1, 2, 2, 1, 1, (16,), ())
    assert not fits(50, 17, 2, 2, 1, 1, (16,), ()) and not fits(50, 0, 2, 2, 1, 1, (16,), ())
    assert fits(50, 1, 1, 1, 1, 1, (512,), (512,)) and not fits(50, 1, 1, 1, 1, 1, (513,), ())
    assert not fits(50, 1, 1, 2, 1, 1, (16,), (513,)) and not fits(50, 1, 1, 2, 1, 1, (0,), ())
    assert fits(50, 1, 2, 2, 1, 1, (8, 8, 8), (8, 8, 8)) and not fits(50, 1, 2, 2, 1, 1, (), ())
    assert not fits(50, 1, 2, 2, 1, 1, (8, 8, 8, 8), ()) and not fits(50, 1, 2, 2, 1, 1, (8,), (8,) * 4)
    # LDS: 16 rows x (nx ldr + 2 ldh + 2 x 72 + gate columns + (K + 1) pad64(H)) floats <= 160 KiB
    assert fits(200, 2, 2, 1, 1, 2, (512, 320), (512,))            # 159,104 B: the op-level `corner` case
    assert not fits(200, 2, 2, 1, 1, 2, (512, 384), (512,))        # 175,488 B
    assert fits(50, 7, 2, 3, 2, 2, (256, 192), ()) and not fits(50, 7, 2, 3, 2, 2, (256, 256), ())
    for c in R.OP_CASES:
        assert fits(c[1], (c[1] + 127) // 128, c[2], c[3], c[4], c[5], c[6], c[7]), c[0]
    assert small_model().fits() and small_model(**R.ALT_CONFIG).fits()


def measured_drifts():
    """float32 against float64 of the restatement at the GPU tests' seeded inputs:
    ([reps, gates, logits, probs] of the ordinary cases and the model cases, the same of extreme_gate).
    The float32 run takes every sum in a fixed order (mmoe_ref.linear), so the figures do not depend on
    the machine's matmul."""
    def over(cases):
        d = [0.0] * 4
        for c in cases:
            o64, o32 = R.flat(R.op_reference(c, torch.float64)), R.flat(R.op_reference(c, torch.float32, ordered=True))
            for i, (a32, a64) in enumerate(zip(o32, o64)):
                d[i] = max([d[i]] + [R.rel_err(x, y) for x, y in zip(a32, a64)])
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
    names = ("REP_TOL", "GATE_TOL", "LOGIT_TOL", "PROB_TOL")
    print("fp32 drift, ordinary:", "  ".join(f"{n} {d:.3g}" for n, d in zip(names, ordinary)))
    print("fp32 drift, extreme_gate:", "  ".join(f"{n} {d:.3g}" for n, d in zip(names, extreme)))
    for n, tol, drift in zip(names, R.tolerances("wechat"), ordinary):
        assert 25 * drift <= tol <= 100 * drift, (n, tol, drift)
    for n, tol, drift in zip(names, R.tolerances(R.EXTREME), extreme):
        assert 25 * drift <= tol <= 100 * drift, ("EXTREME_" + n, tol, drift)


def perturbed_logits(c):
    """The final logits of three wrong computations a kernel could make on the shared path (L >= 2): level
    0's shared gate with zero weights, the own and shared column blocks of a task gate swapped, and level
    1's task gates reading x_s instead of x_k."""
    rows, levels, towers = R.op_inputs(c)
    x = rows[:, :c[1]].double()
    levels, towers = R.cast(levels, torch.float64), R.cast(towers, torch.float64)
    ms = c[4]
    sp, sh, gt, (Ws, bs) = levels[0]
    no_shared_gate = [(sp, sh, gt, (torch.zeros_like(Ws), bs))] + levels[1:]
    W0, b0 = gt[0]
    swapped = [(sp, sh, [(torch.cat([W0[ms:], W0[:ms]]), torch.cat([b0[ms:], b0[:ms]]))] + gt[1:], (Ws, bs))] + levels[1:]
    return {"zero shared gate": R.ple(x, no_shared_gate, towers)[1], "swapped gate blocks": R.ple(x, swapped, towers)[1],
            "task gates read x_s": R.ple(x, levels, towers, task_gates_read_shared=(1,))[1]}


@pytest.mark.parametrize("c", R.OP_CASES, ids=CASE_IDS)
def test_cases_cannot_hide_a_failure(c):
    """On the float64 reference alone: the gates (task and shared alike) are neither uniform nor one-hot,
    extreme_gate is near one-hot, every ReLU clips a fair share (and not all) of its inputs, and a wrong
    shared path moves the logits."""
    name, width, L, K, ms, mc, eu, tu, B = c
    clipped = []
    levels, logits, probs = R.op_reference(c, torch.float64, clipped)
    H_ = eu[-1]
    assert [tuple(lv[0].shape) for lv in levels] == [(B, K + 1, H_)] * (L - 1) + [(B, K, H_)]
    assert all(tuple(lv[1].shape) == (B, K, ms + mc) for lv in levels)
    assert [None if lv[2] is None else tuple(lv[2].shape) for lv in levels] == [(B, K * ms + mc)] * (L - 1) + [None]
    assert logits.shape == probs.shape == (B, K)
    assert len(clipped) == L * (K * ms + mc) * len(eu) + K * len(tu)
    assert all(0.2 <= s <= 0.8 for s in clipped), clipped
    for j, (_, gk, gs) in enumerate(levels):
        for what, g in (("task", gk.reshape(-1, ms + mc)), ("shared", gs)):
            if g is None:
                continue
            top = g.max(dim=-1).values
            mean_top, near_one_hot = float(top.mean()), float((top > 0.95).double().mean())
            print(f"{name} level {j} {what} gates: largest mean {mean_top:.3f}, share above 0.95 {near_one_hot:.3f}")
            if name == R.EXTREME:
                assert near_one_hot > 0.9
            else:
                assert 1.5 / g.shape[-1] <= mean_top <= 0.85, (j, what, mean_top)
                assert near_one_hot <= 0.15, (j, what, near_one_hot)
    print(f"{name}: ReLU clip shares {min(clipped):.2f}-{max(clipped):.2f}")
    assert all(bool(torch.isfinite(t).all()) for group in R.flat((levels, logits, probs)) for t in group)
    if L >= 2:
        tol = R.tolerances(name)[2]
        for what, wrong in perturbed_logits(c).items():
            moved = R.rel_err(wrong, logits)
            print(f"{name}: {what} moves the logits by {moved:.3g} ({moved / tol:.0f} x the tolerance)")
            assert moved > 100 * tol, (what, moved)
