"""GPU tests of DIEN's auxiliary loss: rk_dien_aux_loss(_dense) / rk_dien_aux_loss_backward under
rankops.dien_aux_loss(_gather)'s autograd, the extractor states as a differentiable output of
rankops.dien_interest(_gather) (rk_dien_interest_backward_aux), and
rankops.DIEN(trainable=True, use_auxiliary_loss=True) train steps.

Op oracle: tests/dien_aux_ref.py in float64 on the CPU, differentiated by torch autograd.
Tolerance per tensor: atol = REL * max|want|, rtol 0, exact 0 where the oracle's tensor is all zero;
REL_LOSS / REL_GRAD are fifty times the restatement's own float32 drift on these shapes, measured
and asserted by test_dien_aux_host.py (not tuned on the kernels).

Module oracle: the train-mode restatement of test_gpu_dien_train.py plus the auxiliary loss of its
float32 states, fed the engine's dropout masks; tolerances are _dien_step_check's."""
import pytest
import torch

import dien_aux_ref as R
import dien_ref
import helpers as H
import rankops
import test_gpu_dien_train as tt
from test_gpu_dien import OP_TOL, cuda
from test_gpu_train import _assert_adam_params_close

pytestmark = pytest.mark.gpu

IDS = lambda s: "x".join(map(str, s))  # noqa: E731
CASES = [(s, c, n) for s in R.SHAPES for c in R.CELLS for n in R.T_NEGS]
CASE_IDS = [f"{IDS(s)}-{c}-neg{n}" for s, c, n in CASES]
NEG_KEY = "neg_" + dien_ref.SEQ_KEY


def close(name, got, want, rel):
    shape = tuple(got.shape)
    got = got.double().cpu()
    if want is None:  # the oracle never touched the tensor (the empty negatives of T = 1)
        want = torch.zeros(shape, dtype=torch.float64)
    scale = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    print(f"{name}: max |err| = {err:.3e}, max |want| = {scale:.3e}")
    assert got.shape == want.shape, name
    if scale == 0.0:
        assert (float(got.abs().max()) == 0.0) if got.numel() else True, f"{name}: the oracle's tensor is all zero"
    else:
        assert err <= rel * scale, f"{name}: {err:.3e} > {rel} * {scale:.3e}"


def leaves_of(*ts):
    return [t.cuda().requires_grad_(True) for t in ts]


def run_op_dense(shape, cell, T_neg):
    q, table, ids, neg_ids, lens, w, w_aux, _ = R.case(*shape, T_neg)
    hs = R.op_oracle(*shape, T_neg, cell)[0]
    lv = leaves_of(hs, table[ids], table[neg_ids], w_aux)
    mean, per = rankops.dien_aux_loss(*lv[:3], lens.cuda(), lv[3], return_per_sample=True)
    mean.backward()
    torch.cuda.synchronize()
    return mean.detach(), per.detach(), [t.grad for t in lv]


def run_op_gather(shape, cell, T_neg, ids=None, neg_ids=None):
    q, table, ids0, neg0, lens, w, w_aux, _ = R.case(*shape, T_neg)
    hs = R.op_oracle(*shape, T_neg, cell)[0]
    lv = leaves_of(hs, table, w_aux)
    mean, per = rankops.dien_aux_loss_gather(lv[0], lv[1], (ids0 if ids is None else ids).cuda(),
                                             (neg0 if neg_ids is None else neg_ids).cuda(), lens.cuda(), lv[2],
                                             return_per_sample=True)
    mean.backward()
    torch.cuda.synchronize()
    return mean.detach(), per.detach(), [t.grad for t in lv]


def table_grad(shape, T_neg, dkeys, dneg):
    """The dense table gradient the oracle's row gradients add up to."""
    _, table, ids, neg_ids, *_ = R.case(*shape, T_neg)
    want = torch.zeros(R.VOCAB, shape[2], dtype=torch.float64).index_add_(0, ids.reshape(-1),
                                                                         dkeys.reshape(-1, shape[2]))
    if dneg is not None and dneg.numel():
        want.index_add_(0, neg_ids.reshape(-1), dneg.reshape(-1, shape[2]))
    return want


@pytest.mark.parametrize("shape,cell,T_neg", CASES, ids=CASE_IDS)
def test_dense_and_gather_loss_match_fp64(shape, cell, T_neg):
    B, T, Hd, nh = shape
    lens = R.case(*shape, T_neg)[4]
    _, want_mean, want_per, want = R.op_oracle(*shape, T_neg, cell)
    mean, per, got = run_op_dense(shape, cell, T_neg)
    assert mean.shape == () and per.shape == (B,) and mean.dtype == torch.float32
    close(f"per_sample {shape}", per, want_per, R.REL_LOSS)
    close(f"mean {shape}", mean, want_mean, R.REL_LOSS)
    for n, g, wnt in zip(R.OP_NAMES, got, want):
        assert g is not None and g.dtype == torch.float32, n
        close(f"{n} {shape} {cell} neg{T_neg}", g, wnt, R.REL_GRAD)
    # exact zeros: a sample without a step, key row 0 and rows past the length, negatives of dead steps
    assert float(per.cpu()[lens <= 1].abs().max()) == 0.0 if (lens <= 1).any() else True
    t = torch.arange(T)[None, :]
    dead = (t == 0) | (t >= lens[:, None])
    assert float(got[1].cpu()[dead].abs().max()) == 0.0
    assert float(got[0].cpu()[t >= lens[:, None] - 1].abs().max()) == 0.0
    if T > 1:
        dead_neg = (torch.arange(T - 1)[None, :] >= lens[:, None] - 1).repeat_interleave(T_neg, 1)
        assert float(got[2].cpu()[dead_neg].abs().max()) == 0.0 if dead_neg.any() else True
    gmean, gper, ggot = run_op_gather(shape, cell, T_neg)
    assert torch.equal(gmean, mean) and torch.equal(gper, per)  # one kernel, the same rows
    assert torch.equal(ggot[0], got[0]) and torch.equal(ggot[2], got[3])
    close(f"dtable {shape} {cell} neg{T_neg}", ggot[1], table_grad(shape, T_neg, want[1], want[2]), R.REL_GRAD)
    assert rankops.error_flags() == 0


def run_composition(shape, cell, T_neg, gather=False, use_aux=True):
    B, T, Hd, nh = shape
    q, table, ids, neg_ids, lens, w, w_aux, G = R.case(*shape, T_neg)
    dl, dG = lens.cuda(), G.cuda()
    if gather:
        lv = leaves_of(q, table, *w, w_aux)
        state, hs = rankops.dien_interest_gather(lv[0], lv[1], ids.cuda(), dl, lv[2:11], cell, return_states=True)
        loss = (state * dG).sum() / B
        if use_aux:
            loss = loss + rankops.dien_aux_loss_gather(hs, lv[1], ids.cuda(), neg_ids.cuda(), dl, lv[11])
    else:
        lv = leaves_of(q, table[ids], table[neg_ids], *w, w_aux)
        state, hs = rankops.dien_interest(lv[0], lv[1], dl, lv[3:12], cell, return_states=True)
        loss = (state * dG).sum() / B
        if use_aux:
            loss = loss + rankops.dien_aux_loss(hs, lv[1], lv[2], dl, lv[12])
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), hs.detach(), [t.grad for t in lv]


@pytest.mark.parametrize("shape,cell,T_neg", CASES, ids=CASE_IDS)
def test_composition_with_the_recurrence_matches_fp64_autograd(shape, cell, T_neg):
    """loss = (state * G).sum() / B + aux(hs): the gradient of the auxiliary loss w.r.t. the states
    enters the extractor's backward chain inside the BPTT kernel, and its key gradient adds to
    the recurrence's."""
    B, T, Hd, nh = shape
    want_loss, want = R.composition_oracle(*shape, T_neg, cell)
    loss, hs, got = run_composition(shape, cell, T_neg)
    print(f"loss {shape}: {float(loss):.6f}, want {float(want_loss):.6f}")  # a sum of two signs: printed, not judged
    for n, g, wnt in zip(R.COMP_NAMES, got, want):
        assert g is not None or wnt is None, n
        if g is not None:
            close(f"{n} {shape} {cell} neg{T_neg}", g, wnt, R.REL_GRAD)
    gloss, ghs, ggot = run_composition(shape, cell, T_neg, gather=True)
    assert torch.equal(ghs, hs)
    close(f"dq (gather) {shape}", ggot[0], want[0], R.REL_GRAD)
    close(f"dtable {shape} {cell} neg{T_neg}", ggot[1], table_grad(shape, T_neg, want[1], want[2]), R.REL_GRAD)
    for n, g, wnt in zip(R.COMP_NAMES[3:], ggot[2:], want[3:]):
        close(f"{n} (gather) {shape} {cell} neg{T_neg}", g, wnt, R.REL_GRAD)
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("cell", R.CELLS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=IDS)
def test_unused_states_leave_the_interest_gradients_bit_equal(shape, cell):
    """return_states=True with nothing reading hs: d_hs is absent, the backward is
    rk_dien_interest_backward's, bit for bit; the returned states are zero past the length."""
    B, T, Hd, nh = shape
    q, table, ids, neg_ids, lens, w, w_aux, G = R.case(*shape, 1)
    _, hs, got = run_composition(shape, cell, 1, use_aux=False)
    lv = leaves_of(q, table[ids], *w)
    state = rankops.dien_interest(lv[0], lv[1], lens.cuda(), lv[2:], cell)
    ((state * G.cuda()).sum() / B).backward()
    plain = [t.grad for t in lv]
    for n, x, y in zip(("dq", "dkeys") + R.COMP_NAMES[3:12], [got[0], got[1]] + got[3:12], plain):
        assert torch.equal(x, y), n
    assert got[2] is None and got[12] is None  # negatives and w_aux were not used
    past = torch.arange(T)[None, :] >= lens[:, None]
    assert float(hs.cpu()[past].abs().max()) == 0.0 if past.any() else True
    want_hs = dien_ref.interest(q, table[ids], lens, w, cell)[2]
    torch.testing.assert_close(hs.double().cpu()[~past], want_hs[~past], **OP_TOL)  # the state's own bound
    # under no-grad the train forward kernel hands out the same states, in both forms
    dq, dk, dt, di, dl, dw = cuda(q, table[ids], table, ids, lens, w)
    with torch.no_grad():
        s1, h1 = rankops.dien_interest(dq, dk, dl, dw, cell, return_states=True)
        s2, a2, h2 = rankops.dien_interest_gather(dq, dt, di, dl, dw, cell, return_attention=True, return_states=True)
    assert torch.equal(h1, hs) and torch.equal(h2, hs) and torch.equal(s1, s2) and h1.grad_fn is None
    assert a2.shape == (B, T)


@pytest.mark.parametrize("shape", [(67, 50, 16, 8), (5, 200, 32, 16)], ids=IDS)
def test_two_backward_calls_are_bit_equal(shape):
    for cell in R.CELLS:
        a, b = run_op_dense(shape, cell, 3), run_op_dense(shape, cell, 3)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for n, x, y in zip(R.OP_NAMES, a[2], b[2]):
            assert torch.equal(x, y), (n, cell)
        a, b = run_op_gather(shape, cell, 3), run_op_gather(shape, cell, 3)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for i in (0, 2):  # the table scatter uses float atomics; d_hs and dw_aux do not
            assert torch.equal(a[2][i], b[2][i]), (i, cell)
        a, b = run_composition(shape, cell, 3), run_composition(shape, cell, 3)
        assert torch.equal(a[0], b[0])
        for n, x, y in zip(R.COMP_NAMES, a[2], b[2]):
            assert torch.equal(x, y), (n, cell)


@pytest.mark.parametrize("cell", R.CELLS)
def test_poisoned_ids_at_masked_positions_change_nothing(cell):
    shape, T_neg = (67, 50, 16, 8), 3
    B, T, Hd, nh = shape
    q, table, ids, neg_ids, lens, w, w_aux, G = R.case(*shape, T_neg)
    base = run_op_gather(shape, cell, T_neg)
    bad, bad_neg = ids.clone(), neg_ids.clone()
    bad[torch.arange(T)[None, :] >= lens[:, None]] = 2 ** 40
    bad_neg[(torch.arange(T - 1)[None, :] >= lens[:, None] - 1).repeat_interleave(T_neg, 1)] = 2 ** 40
    assert (bad != ids).any() and (bad_neg != neg_ids).any()
    got = run_op_gather(shape, cell, T_neg, ids=bad, neg_ids=bad_neg)
    assert rankops.error_flags() == 0
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    assert torch.equal(got[2][0], base[2][0]) and torch.equal(got[2][2], base[2][2])
    want = R.op_oracle(*shape, T_neg, cell)[3]
    close("dtable, poisoned ids", got[2][1], table_grad(shape, T_neg, want[1], want[2]), R.REL_GRAD)
    # a bad id at a live position reads a zero row and raises the flag
    live = ids.clone()
    live[0, 1] = R.VOCAB + 5  # sample 0 has the full length
    mean = run_op_gather(shape, cell, T_neg, ids=live)[0]
    assert torch.isfinite(mean) and rankops.error_flags() == rankops._lib.RK_FLAG_INDEX_OOB
    assert rankops.error_flags() == 0


def test_envelope_and_shape_errors():
    shape = (3, 3, 8, 8)
    q, table, ids, neg_ids, lens, w, w_aux, _ = R.case(*shape, 1)
    hs = R.op_oracle(*shape, 1, "AGRU")[0].cuda()
    dt, di, dl, dwa = table.cuda(), ids.cuda(), lens.cuda(), w_aux.cuda()
    nine = torch.zeros(3, 2 * 9, dtype=torch.int64, device="cuda")
    with pytest.raises(NotImplementedError, match="T_neg"):
        rankops.dien_aux_loss_gather(hs, dt, di, nine, dl, dwa)
    with pytest.raises(NotImplementedError, match="T_neg"):
        rankops.dien_aux_loss(hs, dt[di], torch.zeros(3, 18, 8, device="cuda"), dl, dwa)
    with pytest.raises(ValueError, match="multiple of T-1"):
        rankops.dien_aux_loss_gather(hs, dt, di, nine[:, :3], dl, dwa)
    with pytest.raises(ValueError, match="multiple of T-1"):
        rankops.dien_aux_loss(hs, dt[di], torch.zeros(3, 5, 8, device="cuda"), dl, dwa)
    with pytest.raises(ValueError):
        rankops.dien_aux_loss(hs[:, :2], dt[di], dt[neg_ids.cuda()], dl, dwa)
    # the C entry points refuse the same before any launch
    from rankops import ops
    per, mean = torch.empty(3, device="cuda"), torch.empty(1, device="cuda")
    with pytest.raises(rankops.RankOpsError) as e:
        ops.dien_aux_loss(hs, dt, di, None, nine, dl, 3, 9, 8, 8, dwa, per, mean, 3, hs.device)
    assert e.value.code == rankops._lib.RK_ERR_UNSUPPORTED
    assert rankops.error_flags() == 0


# ------------------------------------------------------------------ the module

def build(cfg, seed=42, aux=True):
    torch.manual_seed(seed)
    return rankops.DIEN(None, hidden_units=cfg.get("hidden"), custom_gru_type=cfg.get("cell", "AGRU"),
                        vocab_sizes=H.SMALL_VOCAB, trainable=True, use_auxiliary_loss=aux)


def inputs(cfg, B, seed, T_neg=3):
    inp = tt.inputs(cfg, B, seed)
    T = cfg["T"]
    g = torch.Generator().manual_seed(seed + 1)
    inp["sequence"][NEG_KEY] = torch.randint(0, H.SMALL_VOCAB["feedid"], (B, (T - 1) * T_neg), generator=g)
    return inp


def forward_train_aux(p, inp, cfg, masks):
    """test_gpu_dien_train.py's train-mode restatement, plus the auxiliary loss of the same float32
    states (a second pass of dien_ref.interest: the first keeps its states to itself)."""
    prob, logit, att = tt.dien_forward_train(p, inp, cfg, masks)
    table = p["embeddings.feedid.weight"]
    seq, lens = inp["sequence"][dien_ref.SEQ_KEY], inp["sequence"][f"{dien_ref.SEQ_KEY}_length"]
    keys = torch.nn.functional.embedding(seq, table)
    hs = dien_ref.interest(torch.nn.functional.embedding(inp["target"]["feedid"], table), keys, lens,
                           dien_ref.model_weights(p), cfg.get("cell", "AGRU"), dtype=torch.float32)[2]
    neg = torch.nn.functional.embedding(inp["sequence"][NEG_KEY], table)
    aux = R.aux_loss(hs, keys, neg, lens, p["aux_project_matrix"], dtype=torch.float32)[0]
    return prob, logit, att, aux


@pytest.mark.parametrize("cell", R.CELLS)
def test_dien_train_steps_with_the_auxiliary_loss_match_autograd(cell):
    """Two train steps of loss = bce + aux_loss with rankops.Adam, in the manner (and with the
    tolerances) of test_gpu_dien_train.py::_dien_step_check; aux_project_matrix is judged like the
    other non-embedding parameters."""
    cfg, B, seed = {"T": 8, "cell": cell}, 256, 2600
    model = build(cfg).cuda().train()
    inp = inputs(cfg, B, seed)
    label = (torch.rand(B, generator=torch.Generator().manual_seed(seed)) < 0.3).float()
    params = dict(model.named_parameters())
    assert "aux_project_matrix" in params
    p = {k: (v.detach().cpu().clone().requires_grad_(True) if k in params else v.detach().cpu().clone())
         for k, v in model.state_dict().items()}
    opt = rankops.Adam(model.parameters(), lr=1e-3)
    ref_opt = torch.optim.Adam([p[n] for n in params], lr=1e-3)
    crit = torch.nn.BCELoss()
    dinp = H.to_device(inp, "cuda")
    for step in range(2):
        opt.zero_grad()
        ref_opt.zero_grad()
        out = tt.call(model, dinp, return_attention=True)
        assert len(out) == 4 and out[3].shape == () and out[3].grad_fn is not None and not out[2].requires_grad
        (crit(out[0].squeeze(), label.cuda()) + out[3]).backward()
        r = forward_train_aux(p, inp, cfg, tt._masks(model, B))
        (crit(r[0].squeeze(), label) + r[3]).backward()
        for i, (o, w) in enumerate(zip(out, r)):
            torch.testing.assert_close(o.detach().cpu().reshape(w.shape), w.detach(), rtol=1e-4, atol=1e-4,
                                       msg=lambda m: f"output {i} step {step}: {m}")
        for n, prm in model.named_parameters():
            want = p[n].grad
            assert want is not None and prm.grad is not None, n
            scale = max(1e-3, float(want.abs().max()))
            tol = (5e-3 if n.startswith("embeddings.") else 5e-4) * scale
            torch.testing.assert_close(prm.grad.cpu(), want, rtol=0, atol=tol,
                                       msg=lambda m: f"grad {n} step {step}: {m}")
        opt.step()
        ref_opt.step()
        for n, prm in model.named_parameters():
            _assert_adam_params_close(prm.detach().cpu(), p[n].detach(), lr=1e-3, steps=1,
                                      what=f"param {n} after step {step}")
        with torch.no_grad():  # re-synchronise the oracle to the engine (see _dien_step_check)
            for k, v in model.state_dict().items():
                p[k].copy_(v.cpu())
            for n, prm in model.named_parameters():
                if prm in opt.state and p[n] in ref_opt.state:
                    for key in ("exp_avg", "exp_avg_sq"):
                        ref_opt.state[p[n]][key].copy_(opt.state[prm][key].cpu())
    assert rankops.error_flags() == 0


def test_auxiliary_loss_without_a_gradient_is_skipped_and_inputs_are_validated():
    cfg, B = {"T": 8}, 256
    model = build(cfg).cuda().train()
    inp = inputs(cfg, B, 41)
    dinp = H.to_device(inp, "cuda")
    label = (torch.rand(B, generator=torch.Generator().manual_seed(4)) < 0.3).float().cuda()
    prob, logit, aux = tt.call(model, dinp)
    torch.nn.BCELoss()(prob.squeeze(), label).backward()  # aux unused: its backward does not run
    assert model.aux_project_matrix.grad is None
    assert model.attention_project_matrix.grad is not None
    with torch.no_grad():  # the no-grad train forward still returns the loss (train forward kernel's states)
        p2, l2, a2 = tt.call(model, dinp)
    assert a2.grad_fn is None and torch.equal(a2, aux.detach())
    missing = {k: v for k, v in dinp["sequence"].items() if k != NEG_KEY}
    with pytest.raises(ValueError, match=NEG_KEY):
        model(dinp["dense"], dinp["category"], missing, dinp["target"])
    wrong = dict(dinp["sequence"])
    wrong[NEG_KEY] = wrong[NEG_KEY][:, :-1]
    with pytest.raises(ValueError, match="negative_sample_number"):
        model(dinp["dense"], dinp["category"], wrong, dinp["target"])


def test_graph_captured_step_with_the_auxiliary_loss_matches_eager():
    """test_gpu_dien_train.py's graph test with loss = bce + aux_loss: the auxiliary backward reads
    its upstream scalar from device memory, so the whole step captures; same bounds."""
    cfg = {"T": 8}
    inp = H.to_device(inputs(cfg, 256, seed=31), "cuda")
    label = (torch.rand(256, generator=torch.Generator().manual_seed(31)) < 0.3).float().cuda()
    crit = torch.nn.BCELoss()
    results = []
    for mode in ("eager", "graph"):
        torch.manual_seed(0)
        model = build(cfg).cuda().train()
        opt = rankops.Adam(model.parameters(), lr=1e-3, capturable=True)

        def step():
            opt.zero_grad(set_to_none=False)
            out = tt.call(model, inp)
            (crit(out[0].squeeze(), label) + out[2]).backward()
            opt.step()

        if mode == "eager":
            for _ in range(3):
                step()
        else:
            step()  # allocates the optimizer state
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            g.replay()
            g.replay()
        torch.cuda.synchronize()
        results.append({n: t.detach().cpu().clone() for n, t in model.named_parameters()})
    assert "aux_project_matrix" in results[0]
    for n in results[0]:
        torch.testing.assert_close(results[1][n], results[0][n], rtol=1e-5, atol=1e-6, msg=lambda m: f"{n}: {m}")


def test_flag_on_model_in_eval_equals_the_flag_off_model():
    cfg = {"T": 8}
    on, off = build(cfg).cuda().eval(), build(cfg, aux=False).cuda().eval()
    missing, unexpected = off.load_state_dict(on.state_dict(), strict=False)
    assert not missing and unexpected == ["aux_project_matrix"]
    inp = H.to_device(inputs(cfg, 64, seed=9), "cuda")
    with torch.no_grad():
        a, b = tt.call(on, inp), tt.call(off, inp)
    assert len(a) == 2 and len(b) == 2
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # and a flag-off model in train mode still returns two outputs and ignores the negatives
    assert len(tt.call(off.train(), inp)) == 2
