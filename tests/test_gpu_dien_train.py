"""GPU tests of DIEN training: rk_dien_interest_train(_dense) / rk_dien_interest_backward under
rankops.dien_interest(_gather)'s autograd, and rankops.DIEN(trainable=True) train steps.

Op oracle: tests/dien_ref.py::interest in float64 on the CPU differentiated by torch autograd, loss
(state * G).sum() with a seeded G.  Tolerance per gradient tensor: atol = 4e-5 * max|want|, rtol 0,
exact 0 where the oracle's tensor is all zero.  Not tuned on the kernel: the same restatement
differentiated in fp32 on the CPU stays within 8e-7 of each tensor's largest fp64 gradient on these
shapes (both cells; q, keys and all nine weights); 50 times that drift is the margin
test_gpu_dien.py uses for hardware exp / rcp and another summation order, while a swapped gate, a
missed mask or an off-by-one step shows at 1e-2.

Module oracle: dien_ref.interest plus a train-mode tail (the oracle's din_forward_train tail) fed
the engine's dropout masks; tolerances are those of test_gpu_train.py::_din_step_check."""
import functools

import pytest
import torch
import torch.nn.functional as F

import dien_ref
import helpers as H
import rankops
from oracle import reference_forward as ref
from rankops import _lib, ops
from test_gpu_dien import VOCAB, case, cuda
from test_gpu_train import _assert_adam_params_close

pytestmark = pytest.mark.gpu

CELLS = ("AGRU", "AUGRU")
SHAPES = [(1, 1, 16, 8), (3, 3, 8, 8), (9, 17, 32, 8), (67, 50, 16, 8), (5, 200, 32, 16), (64, 50, 16, 16)]
IDS = lambda s: "x".join(map(str, s))  # noqa: E731
NAMES = ("dq", "dkeys") + tuple("d" + n for n in dien_ref.WEIGHT_NAMES)
REL = 4e-5


def upstream(B, nh, seed=5):
    return torch.randn(B, nh, generator=torch.Generator().manual_seed(seed + B + nh))


@functools.lru_cache(maxsize=None)
def oracle(B, T, Hd, nh, cell):
    """fp64 CPU gradients (dq, dkeys, nine weights) of (state * G).sum(); computed once per case."""
    q, table, ids, lens, w = case(B, T, Hd, nh)
    leaves = [t.double().requires_grad_(True) for t in (q, table[ids], *w)]
    s, _, _ = dien_ref.interest(leaves[0], leaves[1], lens, leaves[2:], cell)
    (s * upstream(B, nh).double()).sum().backward()
    return tuple(t.grad for t in leaves)


def close(name, got, want):
    got = got.double().cpu()
    scale = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    print(f"{name}: max |err| = {err:.3e}, max |want| = {scale:.3e}")
    assert got.shape == want.shape, name
    if scale == 0.0:
        assert float(got.abs().max()) == 0.0 if got.numel() else True, f"{name}: the oracle's gradient is all zero"
    else:
        assert err <= REL * scale, f"{name}: {err:.3e} > {REL} * {scale:.3e}"


def run_dense(shape, cell, G=None):
    B, T, Hd, nh = shape
    q, table, ids, lens, w = case(*shape)
    dq, dk, dl, dw = cuda(q, table[ids], lens, w)
    leaves = [t.requires_grad_(True) for t in (dq, dk, *dw)]
    s = rankops.dien_interest(leaves[0], leaves[1], dl, leaves[2:], cell)
    s.backward(upstream(B, nh).cuda() if G is None else G)
    torch.cuda.synchronize()
    return s.detach(), [t.grad for t in leaves]


def run_gather(shape, cell, ids=None):
    B, T, Hd, nh = shape
    q, table, ids0, lens, w = case(*shape)
    dq, dt, di, dl, dw = cuda(q, table, ids0 if ids is None else ids, lens, w)
    leaves = [t.requires_grad_(True) for t in (dq, dt, *dw)]
    s = rankops.dien_interest_gather(leaves[0], leaves[1], di, dl, leaves[2:], cell)
    s.backward(upstream(B, nh).cuda())
    torch.cuda.synchronize()
    return s.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_dense_gradients_match_fp64_autograd(shape, cell):
    B, T, Hd, nh = shape
    q, table, ids, lens, w = case(*shape)
    want = oracle(*shape, cell)
    s, got = run_dense(shape, cell)
    for n, g, wnt in zip(NAMES, got, want):
        assert g is not None and g.dtype == torch.float32, n
        close(f"{n} {shape} {cell}", g, wnt)
    # the forward under autograd is the no-grad forward
    dq, dk, dl, dw = cuda(q, table[ids], lens, w)
    assert torch.equal(s, rankops.dien_interest(dq, dk, dl, dw, cell))
    # key rows past the length, and every gradient of an empty sample, are exact zeros
    dkeys = got[1].cpu()
    past = torch.arange(T)[None, :] >= lens[:, None]
    assert float(dkeys[past].abs().max()) == 0.0 if past.any() else True
    empty = lens == 0
    if empty.any():
        assert float(got[0].cpu()[empty].abs().max()) == 0.0 and float(dkeys[empty].abs().max()) == 0.0
    if cell == "AGRU":  # the update gate never reaches the output
        assert float(got[2 + 5][nh:].abs().max()) == 0.0 and float(got[2 + 6][nh:].abs().max()) == 0.0
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gather_gradients_match_fp64_autograd(shape, cell):
    B, T, Hd, nh = shape
    q, table, ids, lens, w = case(*shape)
    want = oracle(*shape, cell)
    s, got = run_gather(shape, cell)
    want_table = torch.zeros(VOCAB, Hd, dtype=torch.float64).index_add_(0, ids.reshape(-1), want[1].reshape(-1, Hd))
    close(f"dq {shape} {cell}", got[0], want[0])
    close(f"dtable {shape} {cell}", got[1], want_table)
    for n, g, wnt in zip(NAMES[2:], got[2:], want[2:]):
        close(f"{n} {shape} {cell}", g, wnt)
    dq, dt, di, dl, dw = cuda(q, table, ids, lens, w)
    assert torch.equal(s, rankops.dien_interest_gather(dq, dt, di, dl, dw, cell))
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("shape", [(67, 50, 16, 8), (5, 200, 32, 16)], ids=IDS)
def test_two_backward_calls_are_bit_equal(shape):
    for cell in CELLS:
        _, a = run_dense(shape, cell)
        _, b = run_dense(shape, cell)
        for n, x, y in zip(NAMES, a, b):
            assert torch.equal(x, y), (n, cell)
        _, a = run_gather(shape, cell)
        _, b = run_gather(shape, cell)
        for n, x, y in zip(NAMES[2:], a[2:], b[2:]):  # the table scatter uses float atomics; the rest does not
            assert torch.equal(x, y), (n, cell)
        assert torch.equal(a[0], b[0])


@pytest.mark.parametrize("cell", CELLS)
def test_poisoned_ids_past_the_length_change_no_gradient(cell):
    shape = (67, 50, 16, 8)
    q, table, ids, lens, w = case(*shape)
    _, base = run_gather(shape, cell)
    want = oracle(*shape, cell)
    past = torch.arange(shape[1])[None, :] >= lens[:, None]
    for poison in (VOCAB + 5, -1, 2 ** 40):
        bad = ids.clone()
        bad[past] = poison
        _, got = run_gather(shape, cell, ids=bad)
        assert rankops.error_flags() == 0, poison
        for n, x, y in zip(NAMES[2:], got[2:], base[2:]):
            assert torch.equal(x, y), (n, poison)
        assert torch.equal(got[0], base[0]), poison
        want_table = torch.zeros(VOCAB, shape[2], dtype=torch.float64).index_add_(0, ids.reshape(-1),
                                                                                   want[1].reshape(-1, shape[2]))
        close(f"dtable poison {poison}", got[1], want_table)


@pytest.mark.parametrize("cell", CELLS)
def test_strided_query_and_d_out_in_one_row_buffer(cell):
    """The module's layout: the query and d(state) are columns of one row(-gradient) buffer, and
    dquery is added into the query's columns of the gradient buffer."""
    shape = (67, 50, 16, 8)
    B, T, Hd, nh = shape
    q, table, ids, lens, w = case(*shape)
    want = oracle(*shape, cell)
    dt, di, dl, dw = cuda(table, ids, lens, w)
    width, q_col = 3 + Hd + 5 + nh, 3  # [3 | query | 5 | state]: the query is not 16-B aligned
    row = torch.full((B, width), 777.0, device="cuda")
    row[:, q_col:q_col + Hd] = q.cuda()
    f32 = dict(device="cuda", dtype=torch.float32)
    att, hs, ss = torch.empty(B, T, **f32), torch.empty(B, T, nh, **f32), torch.empty(B, T, nh, **f32)
    c = ops.DIEN_CELLS[cell]
    ops.dien_interest_train(_lib.fptr(row, q_col), width, dt, di, dl, T, Hd, nh, c, dw, _lib.fptr(row, width - nh),
                            width, att, hs, ss, B, row.device)
    assert torch.equal(row[:, width - nh:], rankops.dien_interest(q.cuda(), dt[di], dl, dw, cell))
    assert float(hs.cpu()[torch.arange(T)[None, :] >= lens[:, None]].abs().max()) == 0.0
    drow = torch.full((B, width), 0.25, device="cuda")
    drow[:, width - nh:] = upstream(B, nh).cuda()
    before = drow.clone()
    dkeys = torch.empty(B, T, Hd, **f32)
    wg = ops.dien_interest_backward(_lib.fptr(row, q_col), width, dt, di, 0, dl, T, Hd, nh, c, dw, hs, ss, att,
                                    _lib.fptr(drow, width - nh), width, _lib.fptr(drow, q_col), width, True, dkeys, B,
                                    row.device)
    torch.cuda.synchronize()
    keep = [i for i in range(width) if not q_col <= i < q_col + Hd]
    assert torch.equal(drow[:, keep], before[:, keep])
    close("dq (accumulated)", drow[:, q_col:q_col + Hd] - 0.25, want[0])
    _, plain = run_gather(shape, cell)
    assert torch.equal(dkeys.cpu(), run_dense(shape, cell)[1][1].cpu())
    for n, x, y in zip(NAMES[2:], wg, plain[2:]):
        assert torch.equal(x, y), n


def test_non_contiguous_grad_output_is_accepted():
    shape = (9, 17, 32, 8)
    B, nh = shape[0], shape[3]
    wide = torch.zeros(B, 2 * nh, device="cuda")
    wide[:, ::2] = upstream(B, nh).cuda()
    G = wide[:, ::2]
    assert not G.is_contiguous()
    _, got = run_dense(shape, "AUGRU", G=G)
    for n, g, wnt in zip(NAMES, got, oracle(*shape, "AUGRU")):
        close(n, g, wnt)


def test_plain_tensors_take_the_eval_path():
    q, table, ids, lens, w = case(3, 3, 8, 8)
    dq, dt, di, dl, dw = cuda(q, table, ids, lens, w)
    assert rankops.dien_interest(dq, dt[di], dl, dw).grad_fn is None
    assert rankops.dien_interest_gather(dq, dt, di, dl, dw).grad_fn is None
    with torch.no_grad():
        assert rankops.dien_interest(dq.clone().requires_grad_(True), dt[di], dl, dw).grad_fn is None
    s, a = rankops.dien_interest(dq.clone().requires_grad_(True), dt[di], dl, dw, return_attention=True)
    assert s.grad_fn is not None and not a.requires_grad


# ------------------------------------------------------------------ the module

def build(cfg, seed=42):
    torch.manual_seed(seed)
    return rankops.DIEN(None, hidden_units=cfg.get("hidden"), activation=cfg.get("activation", "dice"),
                        batch_norm=cfg.get("batch_norm", True), custom_gru_type=cfg.get("cell", "AGRU"),
                        gru_output_units=cfg.get("nh", 8), vocab_sizes=H.SMALL_VOCAB,
                        embedding_dim=cfg.get("dim", 16), trainable=True)


def inputs(cfg, B, seed):
    return H.din_inputs(B, cfg.get("T", 20), H.SMALL_VOCAB, seed=seed, min_len=cfg.get("min_len", 1))


def call(m, inp, **kw):
    return m(inp["dense"], inp["category"], inp["sequence"], inp["target"], **kw)


def dien_forward_train(p, inp, cfg, masks, momentum=0.1, eps=1e-5):
    """rankops.DIEN's train-mode forward from its state_dict `p` (requires_grad leaves; the running
    statistics in `p` are updated in place): dien_ref.interest, then the tail of the oracle's
    din_forward_train with the given dropout masks."""
    dense, category, sequence, target = inp["dense"], inp["category"], inp["sequence"], inp["target"]
    cols = [v.reshape(-1, 1) for v in dense.values()]
    cols += [F.embedding(category[f], p[f"embeddings.{f}.weight"]) for f in dien_ref.CATEGORY if f in category]
    table = p["embeddings.feedid.weight"]
    e_target = F.embedding(target["feedid"], table)
    state, att, _ = dien_ref.interest(e_target, F.embedding(sequence[dien_ref.SEQ_KEY], table),
                                      sequence[f"{dien_ref.SEQ_KEY}_length"], dien_ref.model_weights(p),
                                      cfg.get("cell", "AGRU"), dtype=torch.float32)
    net = torch.cat(cols + [e_target, state], 1)
    activation, batch_norm = cfg.get("activation", "dice"), cfg.get("batch_norm", True)
    num_hidden = len(cfg.get("hidden") or [512, 256, 128])
    for u, (lin, act, bn) in enumerate(ref.din_layout(num_hidden, activation, batch_norm, 0.1)):
        net = F.linear(net, p[f"fcn.{lin}.weight"], p[f"fcn.{lin}.bias"])
        if activation == "dice":
            net = ref.dice_train(net, p, f"fcn.{act}.", momentum, eps)
        else:
            net = F.prelu(net, p[f"fcn.{act}.weight"])
        if bn is not None:
            pre = f"fcn.{bn}."
            net = F.batch_norm(net, p[pre + "running_mean"], p[pre + "running_var"], p[pre + "weight"],
                               p[pre + "bias"], training=True, momentum=momentum, eps=eps)
            p[pre + "num_batches_tracked"] += 1
        if masks is not None and masks[u] is not None:
            net = net * masks[u]
    logit = F.linear(net, p["output_layer.weight"], p["output_layer.bias"])
    return torch.sigmoid(logit), logit, att


def _masks(model, B):
    from rankops import train as rt
    slot = model._dropout.counter - 1
    return [ops.dropout_mask(model._dropout.seed + u, slot, B, lin.out_features, p).cpu() if p > 0 else None
            for u, (lin, act, bn, p) in enumerate(rt.din_units(model))]


def _dien_step_check(cfg, B, seed, steps):
    """DIEN train steps (dien.py:314-334: forward, sigmoid cross-entropy, Adam) against the oracle
    differentiated by autograd with the dropout masks the engine drew; tolerances of _din_step_check."""
    model = build(cfg).cuda().train()
    inp = inputs(cfg, B, seed)
    label = (torch.rand(B, generator=torch.Generator().manual_seed(seed)) < 0.3).float()
    params = dict(model.named_parameters())
    p = {k: (v.detach().cpu().clone().requires_grad_(True) if k in params else v.detach().cpu().clone())
         for k, v in model.state_dict().items()}
    opt = rankops.Adam(model.parameters(), lr=1e-3)
    ref_opt = torch.optim.Adam([p[n] for n in params], lr=1e-3)
    crit = torch.nn.BCELoss()
    dinp = H.to_device(inp, "cuda")
    for step in range(steps):
        opt.zero_grad()
        ref_opt.zero_grad()
        out = call(model, dinp, return_attention=True)
        assert out[0].grad_fn is not None and not out[2].requires_grad
        crit(out[0].squeeze(), label.cuda()).backward()
        r = dien_forward_train(p, inp, cfg, _masks(model, B))
        crit(r[0].squeeze(), label).backward()
        for i, (o, w) in enumerate(zip(out, r)):
            torch.testing.assert_close(o.detach().cpu().reshape(w.shape), w.detach(), rtol=1e-4, atol=1e-4,
                                       msg=lambda m: f"output {i} step {step}: {m}")
        for k, v in model.state_dict().items():
            if k not in params and (step == 0 or not k.endswith("running_mean")):
                torch.testing.assert_close(v.cpu(), p[k], rtol=1e-4, atol=1e-5,
                                           msg=lambda m: f"buffer {k} step {step}: {m}")
        for n, prm in model.named_parameters():
            want = p[n].grad
            if want is None:
                assert prm.grad is None or float(prm.grad.abs().max()) == 0.0, n
                continue
            scale = max(1e-3, float(want.abs().max()))
            tol = (5e-3 if n.startswith("embeddings.") else 5e-4) * scale
            torch.testing.assert_close(prm.grad.cpu(), want, rtol=0, atol=tol,
                                       msg=lambda m: f"grad {n} step {step}: {m}")
        opt.step()
        ref_opt.step()
        for n, prm in model.named_parameters():
            if p[n].grad is not None:
                _assert_adam_params_close(prm.detach().cpu(), p[n].detach(), lr=1e-3, steps=1,
                                          what=f"param {n} after step {step}")
        with torch.no_grad():  # re-synchronise the oracle to the engine (see _deepfm_step_check)
            for k, v in model.state_dict().items():
                p[k].copy_(v.cpu())
            for n, prm in model.named_parameters():
                if prm in opt.state and p[n] in ref_opt.state:
                    for key in ("exp_avg", "exp_avg_sq"):
                        ref_opt.state[p[n]][key].copy_(opt.state[prm][key].cpu())
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("cfg", [{"T": 20}, {"T": 20, "cell": "AUGRU"},
                                 {"T": 12, "activation": "prelu", "batch_norm": False},
                                 {"T": 20, "nh": 16, "dim": 32, "hidden": [64, 32], "cell": "AUGRU"},
                                 {"T": 70, "min_len": 0}],
                         ids=["agru", "augru", "prelu_no_bn", "nh16_dim32", "long_empty"])
def test_dien_train_steps_match_autograd(cfg):
    _dien_step_check(cfg, 256, seed=2500, steps=2)


def test_dien_train_graph_capture_matches_eager():
    """A whole DIEN train step (capturable Adam) captured in one hipGraph gives the same parameters
    as three eager steps.  Both sides run rankops.Adam(capturable=True): its kernel takes the bias
    corrections from a device step counter in fp32 (as torch's capturable Adam does), the
    host-stepped kernel in double, and that rounding alone, normalised by Adam on small-gradient
    elements, moves single elements by up to 4e-6 in three steps (measured: eager capturable against
    the captured graph differs by 1.2e-7, one ulp of the atomically scattered embedding
    gradients); the two Adam kernels are compared in test_gpu_train.py."""
    cfg = {"T": 20}
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
            out = call(model, inp)
            crit(out[0].squeeze(), label).backward()
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
    for n in results[0]:
        torch.testing.assert_close(results[1][n], results[0][n], rtol=1e-5, atol=1e-6, msg=lambda m: f"{n}: {m}")


def test_eval_after_train_steps_uses_the_updated_running_statistics():
    cfg = {"T": 20}
    model = build(cfg).cuda()
    inp = inputs(cfg, 256, seed=77)
    dinp = H.to_device(inp, "cuda")
    label = (torch.rand(256, generator=torch.Generator().manual_seed(3)) < 0.3).float().cuda()
    model.eval()
    with torch.no_grad():
        before = call(model, dinp)[1].clone()
    model.train()
    opt = rankops.Adam(model.parameters(), lr=1e-3)
    for _ in range(2):
        opt.zero_grad()
        torch.nn.BCELoss()(call(model, dinp)[0].squeeze(), label).backward()
        opt.step()
    model.eval()
    with torch.no_grad():
        after = call(model, dinp)[1]
    want = dien_ref.forward(H.cpu_params(model), inp["dense"], inp["category"], inp["sequence"], inp["target"])
    torch.testing.assert_close(after.double().cpu(), want[1], atol=1e-4, rtol=1e-4)
    assert float((after - before).abs().max()) > 1e-3  # batch statistics replaced the initial 0 / 1


def test_train_mode_forward_under_no_grad_keeps_nothing():
    cfg = {"T": 20}
    model = build(cfg).cuda().train()
    inp = inputs(cfg, 256, seed=78)
    dinp = H.to_device(inp, "cuda")
    p = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        prob, logit, att = call(model, dinp, return_attention=True)
    assert prob.grad_fn is None and logit.grad_fn is None and not prob.requires_grad
    with torch.no_grad():
        want = dien_forward_train(p, inp, cfg, _masks(model, 256))
    torch.testing.assert_close(logit.cpu(), want[1], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(att.cpu(), want[2], rtol=1e-4, atol=1e-4)
    for k, v in model.state_dict().items():  # batch statistics were used and the running ones updated
        if k.endswith("running_var"):
            torch.testing.assert_close(v.cpu(), p[k], rtol=1e-4, atol=1e-5, msg=k)
