"""CPU checks of the PLE training restatement (tests/ple_train_ref.py): that it is ple_ref's function in
eval, that its gradients are right (gradcheck, and the written-out per-row backward of one level that
rk_ple_mix_backward states), that the tolerances follow from its own float32 drift, that the seeded cases
could not hide a backward that lost one of PLE's own paths, and that the training flags leave the module's
parameters alone.  No GPU."""
import sys

import pytest
import torch

import ple_ref as R
import ple_train_ref as T

ORDINARY = [c for c in T.GRAD_CASES if c[0] != R.EXTREME]
ALL_TERMS = ("reps", "logits", "probs")


@pytest.mark.parametrize("c", T.GRAD_CASES, ids=[c[0] for c in T.GRAD_CASES])
def test_eval_restatement_is_ple_ref_bit_for_bit(c):
    rows, levels, towers = T.op_inputs(c)
    for dtype in (torch.float64, torch.float32):
        x, lv, tw = rows[:, :c[1]].to(dtype), R.cast(levels, dtype), R.cast(towers, dtype)
        want, got = R.ple(x, lv, tw), T.ple(x, lv, tw)
        for a, b in zip([t for g in R.flat(want) for t in g], [t for g in R.flat(got) for t in g]):
            assert torch.equal(a, b), c[0]


def test_gradcheck_on_a_tiny_case():
    c = ("tiny", 5, 2, 2, 1, 1, (4, 3), (3,), 3)
    rows, levels, towers = R.op_inputs(c, 7)
    keeps = T.cpu_keeps(T.sites_of(*c[2:8]), c[8], 0.3)
    leaves = T.leaves((rows[:, :c[1]], levels, towers), torch.float64)
    tensors = T.flat(leaves)

    def f(*ts):
        it = iter(ts)
        rebuild = lambda o: None if o is None else next(it) if isinstance(o, torch.Tensor) else type(o)(rebuild(i) for i in o)  # noqa: E731
        x, lv, tw = rebuild(leaves)
        out, logits, probs = T.ple(x, lv, tw, keeps)
        return out[-1][0], logits, probs
    assert torch.autograd.gradcheck(f, tensors, eps=1e-6, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("K,ms,mc,last", [(3, 2, 2, False), (2, 1, 3, True), (2, 0, 1, True), (1, 2, 1, False)])
def test_one_levels_mix_and_gate_backward_written_out_per_row(K, ms, mc, last):
    """dg_i[c] = sum_h dm_i[h] f_{s(i,c)}[h];  dgl_i[c] = g_i[c] (dg_i[c] - sum_c' g_i[c'] dg_i[c']);
    dz_s[h] = (sum over (i, c) with s(i, c) = s of g_i[c] dm_i[h]) mask_scale [f_s[h] > 0] — the contract of
    rk_ple_mix_backward — against autograd through softmax, the mixtures, ReLU and the keep-multiplier."""
    B, H, p = 4, 5, 0.25
    NE, GT, nq = K * ms + mc, ms + mc, K + (not last)
    g = torch.Generator().manual_seed(100 * K + 10 * ms + mc)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    zf = rnd(B, NE, H).requires_grad_(True)                     # the stacks' last pre-activations
    keep = (torch.rand(B, NE, H, generator=g, dtype=torch.float64) >= p).double() / (1 - p)
    zg = [rnd(B, GT if i < K else NE).requires_grad_(True) for i in range(nq)]
    dm = rnd(B, nq, H)
    stack_of = lambda i, c: c if i == K else (i * ms + c if c < ms else K * ms + c - ms)  # noqa: E731
    f = torch.relu(zf) * keep
    gs = [torch.softmax(z, dim=1) for z in zg]
    loss = sum((dm[:, i] * sum(gs[i][:, c:c + 1] * f[:, stack_of(i, c)] for c in range(gs[i].shape[1]))).sum()
               for i in range(nq))
    loss.backward()
    fd, scale = f.detach(), 1 / (1 - p)
    for b in range(B):
        dz = torch.zeros(NE, H, dtype=torch.float64)
        for i in range(nq):
            gi = gs[i][b].detach()
            dg = torch.stack([(dm[b, i] * fd[b, stack_of(i, c)]).sum() for c in range(len(gi))])
            dgl = gi * (dg - (gi * dg).sum())
            assert torch.allclose(dgl, zg[i].grad[b], rtol=1e-12, atol=1e-13)
            if len(gi) == 1:
                assert float(dgl.abs().max()) < 1e-15
            for c in range(len(gi)):
                dz[stack_of(i, c)] += gi[c] * dm[b, i]
        dz = dz * scale * (fd[b] > 0)
        assert torch.allclose(dz, zf.grad[b], rtol=1e-12, atol=1e-13)


def test_flags_add_no_parameter_and_keep_the_seeded_values():
    import rankops
    plain = T.build_model({})
    flagged = T.build_model({}, trainable=True, sparse_grad=True)
    sa, sb = plain.state_dict(), flagged.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert [n for n, _ in plain.named_parameters()] == [n for n, _ in flagged.named_parameters()]
    assert flagged.trainable and flagged.sparse_grad and not plain.trainable and not plain.sparse_grad
    alt = T.build_model(R.ALT_CONFIG, trainable=True)
    assert list(alt.state_dict()) == list(R.build_model(("x", "small", 1, R.ALT_CONFIG)).state_dict())
    assert "(j * NE + s) * De + l" in sys.modules[rankops.PLE.__module__].__doc__  # the dropout sites are documented


def test_tolerances_are_50x_the_measured_drift():
    d = T.drifts()
    consts = {"ordinary": (T.DX_TOL, T.DW_TOL, T.DGATE_TOL),
              "extreme": (T.EXTREME_DX_TOL, T.EXTREME_DW_TOL, T.EXTREME_DGATE_TOL)}
    for which, tols in consts.items():
        for name, tol, drift in zip(("dx", "dw", "dgate"), tols, d[which]):
            print(f"{which} {name}: drift {drift:.3e}, tolerance {tol:.1e} = {tol / drift:.1f} x")
            assert 25 * drift <= tol <= 100 * drift, (which, name, drift, tol)


# ---------------------------------------------------------------- the seeded cases cannot hide a failure

def _full(c, wrong=None):
    rows, levels, towers = T.op_inputs(c)
    return T.op_gradients(rows[:, :c[1]], levels, towers, use=ALL_TERMS, wrong=wrong)


_FULL = {}


def full_reference(c):
    if c[0] not in _FULL:
        _FULL[c[0]] = _full(c)
    return _FULL[c[0]]


FLOOR_CASES = [c for c in ORDINARY if c[8] >= 16]


@pytest.mark.parametrize("c", FLOOR_CASES, ids=[c[0] for c in FLOOR_CASES])
def test_every_gate_and_every_first_layer_has_a_gradient_of_ordinary_size(c):
    name, width, L, K, ms, mc, eu, tu, B = c
    ref = full_reference(c)
    NE, De = K * ms + mc, len(eu)
    gate_w = ref["gates"][0::2]
    assert len(gate_w) == L * (K + 1) - 1
    smallest_gate = min(float(g.abs().max()) for g in gate_w)
    first = [ref["experts"][2 * ((j * NE + s) * De)] for j in range(L) for s in range(NE)]
    assert all(w.shape == (eu[0], width if i < NE else eu[-1]) for i, w in enumerate(first))
    smallest_first = min(float(w.abs().max()) for w in first)
    print(f"{name}: smallest largest gate weight gradient {smallest_gate:.3f}, first-layer {smallest_first:.3f}")
    assert smallest_gate >= 0.05 and smallest_first >= 0.05


WRONG_CASES = [(c, w) for c in T.GRAD_CASES if c[2] >= 2 and c[8] >= 16 for w in T.WRONG
               if not (w == "last_shared_to_task0" and c[3] < 2)]


@pytest.mark.parametrize("c,wrong", WRONG_CASES, ids=[f"{c[0]}-{w}" for c, w in WRONG_CASES])
def test_a_backward_that_lost_a_path_moves_a_gradient_far_beyond_its_tolerance(c, wrong):
    ref, bad = full_reference(c), _full(c, wrong)
    for a, b in zip(R.flat(ref["out"]), R.flat(bad["out"])):  # the forward is untouched
        assert all(torch.equal(s, t) for s, t in zip(a, b))
    dx, dw, dgate = T.tolerances(c[0])
    ratios = [R.rel_err(bad["dx"], ref["dx"]) / dx]
    ratios += [R.rel_err(a, b) / dw for a, b in zip(bad["experts"] + bad["towers"], ref["experts"] + ref["towers"])]
    ratios += [R.rel_err(a, b) / dgate for a, b in zip(bad["gates"], ref["gates"])]
    print(f"{c[0]} {wrong}: largest change {max(ratios):.0f} x its tolerance")
    assert max(ratios) > 100
