"""ESMM training on the GPU: rk_esmm_loss and rankops.esmm_loss, rk_esmm_joint_backward, differentiable
rankops.esmm and ESMM(trainable=True), against the float64 restatements (tests/esmm_ref.py for the loss,
tests/esmm_train_ref.py for the gradients, which state the tolerances and where they come from)."""
import itertools

import pytest
import torch

import esmm_ref as R
import esmm_train_ref as T
import helpers as H
import rankops
from rankops import _lib, ops
from test_gpu_train import _assert_adam_params_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.0
INVALID = 1  # RK_ERR_INVALID (include/rankops.h)


def close(got, ref, tol, what):
    err = R.rel_err(got, ref)
    print(f"{what}: rel err {err:.3e} (tolerance {tol:.1e})")
    assert bool(torch.isfinite(got).all()), what
    assert got.shape == ref.shape and err <= tol, f"{what}: {err:.3e} > {tol:.1e}"


def to_gpu(obj, grad):
    if obj is None:
        return None
    if isinstance(obj, torch.Tensor):
        return obj.to(DEV).requires_grad_(grad)
    return type(obj)(to_gpu(o, grad) for o in obj)


# ---------------------------------------------------------------- the loss

def run_loss(lc):
    """rk_esmm_loss through ops.esmm_loss_launch on the padded buffers of a loss case."""
    B, K, _, w = lc
    zb, yb = (t.to(DEV) for t in R.loss_inputs(lc))
    loss, per_task = torch.full((), SENTINEL, device=DEV), torch.full((K,), SENTINEL, device=DEV)
    dbuf = torch.full((B, K + 2), SENTINEL, device=DEV)
    ops.esmm_loss_launch(zb[:, :K], yb[:, :K], w, loss, per_task, dbuf[:, :K])
    torch.cuda.synchronize()
    assert bool((dbuf[:, K:] == SENTINEL).all())  # the pad columns of the gradient buffer are not written
    return loss, per_task, dbuf[:, :K]


@pytest.mark.parametrize("lc", R.LOSS_CASES, ids=[f"B{c[0]}_K{c[1]}_s{int(c[2])}" for c in R.LOSS_CASES])
def test_loss_matches_float64(lc):
    B = lc[0]
    loss, per_task, dz = run_loss(lc)
    ref = R.loss_reference(lc)
    lt, tt, dt = R.loss_tolerances(lc[2])
    close(loss, ref[0], lt, f"{lc} loss")
    close(per_task, ref[1], tt, f"{lc} per-task means")
    close(dz * B, ref[2] * B, dt, f"{lc} B * dlogits")
    again = run_loss(lc)
    assert all(torch.equal(a, b) for a, b in zip((loss, per_task, dz), again))  # fixed-order sums, no atomics


def test_loss_is_finite_at_extreme_logits_and_zero_on_an_empty_batch():
    """Logits of +-200: every output must be finite (S_k is clamped where it feeds expm1 / log1mexp).
    Finiteness only: no accuracy is claimed at this magnitude."""
    z = torch.tensor([[200.0, 200.0, 200.0], [-200.0, 200.0, -200.0], [200.0, -200.0, 200.0], [-200.0, -200.0, -200.0]],
                     device=DEV)
    for y in ([[1.0, 0.0, 0.0]] * 4, [[1.0, 1.0, 1.0]] * 4, [[0.0, 0.0, 0.0]] * 4):
        loss, per_task = torch.empty((), device=DEV), torch.empty(3, device=DEV)
        dz = torch.empty(4, 3, device=DEV)
        ops.esmm_loss_launch(z, torch.tensor(y, device=DEV), (1.0, 3.0, 0.5), loss, per_task, dz)
        assert all(bool(torch.isfinite(t).all()) for t in (loss, per_task, dz)), y
    z0 = torch.zeros(0, 3, device=DEV, requires_grad=True)
    loss, per_task = rankops.esmm_loss(z0, torch.zeros(0, 3, device=DEV), return_per_task=True)
    assert float(loss) == 0.0 and bool((per_task == 0).all())
    loss.backward()
    assert z0.grad.shape == (0, 3)


def test_esmm_loss_under_autograd_with_an_upstream_gradient():
    lc = R.LOSS_CASES[2]
    B, K, _, w = lc
    zb, yb = (t.to(DEV) for t in R.loss_inputs(lc))
    z = zb[:, :K].clone().requires_grad_(True)
    loss, per_task = rankops.esmm_loss(z, yb[:, :K], w, return_per_task=True)
    assert loss.dim() == 0 and loss.requires_grad and not per_task.requires_grad
    (loss * 2.5).backward()
    ref = R.loss_reference(lc)
    lt, tt, dt = R.loss_tolerances(lc[2])
    close(loss.detach(), ref[0], lt, "esmm_loss")
    close(per_task, ref[1], tt, "esmm_loss per task")
    close(z.grad * B / 2.5, ref[2] * B, dt, "esmm_loss gradient")
    with torch.no_grad():
        quiet = rankops.esmm_loss(z, yb[:, :K], w)
    assert torch.equal(quiet, loss.detach()) and quiet.grad_fn is None
    with pytest.raises(ValueError):
        rankops.esmm_loss(z, yb[:, :K + 1])
    # raw envelope
    lib = _lib.load()
    out = torch.full((1,), SENTINEL, device=DEV)
    ws = torch.empty(64, device=DEV)
    call = lambda K_=K, ld=K, ws_n=64: lib.rk_esmm_loss(z.data_ptr(), ld, yb.data_ptr(), yb.stride(0), B, K_, None,  # noqa: E731
                                                        out.data_ptr(), None, None, 0, ws.data_ptr(), ws_n,
                                                        _lib.raw_stream(DEV))
    assert call(K_=9, ld=9) == _lib.RK_ERR_UNSUPPORTED and "rk_esmm_loss" in _lib.last_error()
    assert call(ld=K - 1) == INVALID and call(ws_n=1) == INVALID
    torch.cuda.synchronize()
    assert float(out) == SENTINEL


# ---------------------------------------------------------------- the fold onto the logits

SUBSETS = [s for r in (1, 2, 3) for s in itertools.combinations(("probs", "logits", "cond"), r)]


@pytest.mark.parametrize("use", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_joint_backward_matches_autograd(use):
    for lc in (R.LOSS_CASES[2], R.LOSS_CASES[4]):
        K = lc[1]
        z = R.loss_inputs(lc)[0][:, :K].contiguous()
        inc, ref = T.joint_gradients(z, use)
        g = {n: inc[n].float().to(DEV) if n in inc else None for n in ("probs", "logits", "cond")}
        got = ops.esmm_joint_backward(z.to(DEV), g["logits"], g["probs"], g["cond"], _lib.raw_stream(DEV))
        close(got, ref, T.JOINT_TOL, f"joint backward {use} K={K}")
    lib = _lib.load()
    out = torch.full((4, 2), SENTINEL, device=DEV)
    zz = torch.zeros(4, 2, device=DEV)
    assert lib.rk_esmm_joint_backward(zz.data_ptr(), 2, None, None, None, 2, 4, 2, out.data_ptr(), 2,
                                      _lib.raw_stream(DEV)) == INVALID
    assert "rk_esmm_joint_backward" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------- op level

def run_op(c, pad=R.ROW_PAD, use=("probs", "logits", "cond"), bias=True):
    """Differentiable rankops.esmm on one case; returns T.op_gradients' dict of GPU results."""
    rows, towers = T.op_inputs(c)
    width = c[1]
    if not bias:
        towers = [([(w, None) for w, _ in hidden], (w, None)) for hidden, (w, _) in towers]
    xb = rows[:, :width + pad].contiguous().to(DEV).requires_grad_(True)
    gt = to_gpu(towers, True)
    out = rankops.esmm(xb[:, :width], gt, return_conditional=True)
    assert all(o.grad_fn is not None for o in out)
    B, K = out[0].shape
    loss = torch.zeros((), device=DEV)
    for name, cf, o in zip(("probs", "logits", "cond"), T.loss_coeffs(B, K), out):
        if name in use:
            loss = loss + (cf.float().to(DEV) * o).sum()
    loss.backward()
    grads = lambda ts: [t.grad if t.grad is not None else torch.zeros_like(t) for t in ts]  # noqa: E731
    return dict(out=tuple(o.detach() for o in out), dx=xb.grad[:, :width], pad=xb.grad[:, width:], towers=grads(T.flat(gt)))


def compare(got, ref, name, what=""):
    """Every gradient against the restatement; all figures are printed before the first failure is raised."""
    assert len(got["towers"]) == len(ref["towers"])
    items = [(got["dx"], ref["dx"], T.DX_TOL, "dx")]
    items += [(a, b, T.DW_TOL, f"tower grad {i}") for i, (a, b) in enumerate(zip(got["towers"], ref["towers"]))]
    bad = []
    for a, b, tol, what_ in items:
        err = R.rel_err(a, b)
        print(f"{name}{what} {what_}: rel err {err:.3e} (tolerance {tol:.1e})")
        if a.shape != b.shape or not err <= tol:
            bad.append(f"{what_}: {err:.3e} > {tol:.1e}")
    assert not bad, f"{name}{what}: " + "; ".join(bad)


@pytest.mark.parametrize("c", T.GRAD_CASES, ids=[c[0] for c in T.GRAD_CASES])
def test_op_gradients_match_restatement(c):
    ref = T.op_reference(c)
    got = run_op(c)
    lt, pt, ct = R.tolerances(c[0])
    for o, r, t, n in zip(got["out"], ref["out"], (pt, lt, ct), ("probs", "logits", "cond")):
        close(o, r, t, f"{c[0]} {n}")
    compare(got, ref, c[0])
    assert bool((got["pad"] == 0).all())  # the pad columns of the row buffer take no gradient
    again = run_op(c)                      # no atomics, fixed-order sums
    assert torch.equal(got["dx"], again["dx"]) and all(torch.equal(a, b) for a, b in zip(got["towers"], again["towers"]))
    assert rankops.error_flags() == 0


def test_op_single_outputs_missing_biases_eval_bits_and_empty_batch():
    c = R.case("odd")
    rows, towers = T.op_inputs(c)
    x = rows[:, :c[1]]
    for use in (("probs",), ("logits",), ("cond",)):
        compare(run_op(c, use=use), T.op_gradients(x, towers, use=use), "odd", f" ({use[0]} alone)")
    nb = [([(w, None) for w, _ in hidden], (w, None)) for hidden, (w, _) in towers]
    got = run_op(c, bias=False)
    assert len(got["towers"]) == c[2] * (len(c[3]) + 1)
    compare(got, T.op_gradients(x, nb), "odd", " (no biases)")
    # without grad the call is the eval launch; the train forward without dropout has its bits
    xg = x.to(DEV)
    plain = rankops.esmm(xg, to_gpu(towers, False), return_conditional=True)
    assert all(o.grad_fn is None and not o.requires_grad for o in plain)
    tracked = run_op(c)["out"]
    with torch.no_grad():
        quiet = rankops.esmm(xg, to_gpu(towers, True), return_conditional=True)
    for a, b, q in zip(plain, tracked, quiet):
        assert torch.equal(a, b) and torch.equal(a, q) and q.grad_fn is None
    gt = to_gpu(towers, True)
    x0 = torch.zeros(0, c[1], device=DEV, requires_grad=True)
    out = rankops.esmm(x0, gt)
    assert out[0].shape == (0, c[2])
    (out[0].sum() + out[1].sum()).backward()
    assert x0.grad.shape == (0, c[1]) and all(bool((w.grad == 0).all()) for w in T.flat(gt))


def test_train_forward_envelope():
    lib = _lib.load()
    dev = torch.device(DEV)
    _lib.ensure_device(dev)
    width, K, n = 20, 2, 16
    x = torch.ones(4, width, device=DEV)
    img = [torch.zeros(64, 64, device=DEV) for _ in range(K)]
    heads = [(torch.zeros(n, device=DEV), torch.zeros(1, device=DEV)) for _ in range(K)]
    args, keep = ops.esmm_forward_args([ops.dense_segment(x, width, 0)], width, 4, [[(img[k], None, n, "relu")] for k in range(K)],
                                       heads, dev)
    xo, ta = torch.full((4, width), SENTINEL, device=DEV), torch.full((4, K * n), SENTINEL, device=DEV)
    lg = torch.full((4, K), SENTINEL, device=DEV)

    def call(p=0.0, xo_=xo.data_ptr(), ta_=ta.data_ptr()):
        return lib.rk_esmm_forward_train(*args[:9], p, 0, None, xo_, ops._ptrs([ta_]), lg.data_ptr(), None, None,
                                         _lib.raw_stream(dev))
    assert call(xo_=None) == INVALID and "rk_esmm_forward_train" in _lib.last_error()
    assert call(p=0.5) == INVALID          # dropout without a stream slot
    assert call(ta_=ta.data_ptr() + 4) == INVALID
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (xo, ta, lg))
    assert call() == _lib.RK_OK
    assert bool((xo == 1).all()) and bool((ta == 0).all()) and bool((lg == 0).all())


# ---------------------------------------------------------------- the model

def engine_keeps(model, B):
    """The dropout multipliers the last train forward drew, by the documented site numbering."""
    slot = model._dropout.counter - 1
    sites = T.sites_of(len(model.task_names), model.tower_hidden_units)
    return {s: ops.dropout_mask(model._dropout.seed + s, slot, B, n, model.dropout_rate).cpu().double() for s, n in sites}


def model_loss(probs, logits):
    cp, cl, _ = (t.float().to(logits.device) for t in T.loss_coeffs(*logits.shape))
    return (cp * probs).sum() + (cl * logits).sum()


def is_table(name):
    return name.startswith("embeddings.")


@pytest.mark.parametrize("mc", T.MODEL_CASES, ids=[m[0] for m in T.MODEL_CASES])
def test_model_gradients_match_restatement_with_the_engines_masks(mc):
    _, B, kw = mc
    model = T.build_model(kw, trainable=True).to(DEV).train()
    p64 = R.floats(H.cpu_params(model), torch.float64)
    dense, cat = T.model_inputs(B)
    torch.manual_seed(11)
    probs, logits = model(dense.to(DEV), H.to_device(cat, DEV))
    assert probs.requires_grad and logits.requires_grad and probs.shape == (B, len(model.task_names))
    model_loss(probs, logits).backward()
    keeps = engine_keeps(model, B)
    for s, k in keeps.items():  # every site keeps about 1 - p of its elements
        assert abs(float((k > 0).double().mean()) - 0.9) < 0.1, s
    rp, rl, ref = T.model_gradients(p64, dense, cat, keeps=keeps)
    close(logits.detach(), rl, R.LOGIT_TOL, "train logits")
    close(probs.detach(), rp, R.PROB_TOL, "train probs")
    tol = (T.DX_TOL, T.DW_TOL)
    for name, prm in model.named_parameters():
        assert prm.grad is not None, name
        close(prm.grad, ref[name], tol[T.group_of(name)], f"grad {name}")
    # a second forward draws other masks; the same seed on a fresh model repeats the first
    p2, _ = model(dense.to(DEV), H.to_device(cat, DEV))
    assert not torch.equal(p2.detach(), probs.detach())
    twin = T.build_model(kw, trainable=True).to(DEV).train()
    torch.manual_seed(11)
    p3, l3 = twin(dense.to(DEV), H.to_device(cat, DEV))
    assert torch.equal(p3.detach(), probs.detach())
    model_loss(p3, l3).backward()
    for (name, a), b in zip(model.named_parameters(), twin.parameters()):
        if is_table(name):  # rk_embedding_backward adds duplicate ids with float atomics: order-dependent rounding
            close(b.grad, a.grad.cpu().double(), T.DX_TOL, f"repeat grad {name}")
        else:
            assert torch.equal(a.grad, b.grad), f"repeat grad {name}"
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("kw", [{}, R.ALT_CONFIG], ids=["default", "alt"])
def test_model_without_dropout_has_the_eval_bits_and_no_grad_saves_nothing(kw):
    B = 300
    model = T.build_model(dict(kw, dropout_rate=0.0), trainable=True).to(DEV)
    dense, cat = T.model_inputs(B)
    d, c = dense.to(DEV), H.to_device(cat, DEV)
    with torch.no_grad():
        ep, el = model.eval()(d, c)
    tp, tl = model.train()(d, c)
    assert torch.equal(tp.detach(), ep) and torch.equal(tl.detach(), el)
    with torch.no_grad():
        qp, ql = model(d, c)
    assert qp.grad_fn is None and not ql.requires_grad and torch.equal(qp, ep) and torch.equal(ql, el)
    # with dropout: no_grad in train mode returns what the tracking forward returns under one seed
    model = T.build_model(kw, trainable=True).to(DEV).train()
    torch.manual_seed(3)
    a = model(d, c)[1].detach()
    twin = T.build_model(kw, trainable=True).to(DEV).train()
    torch.manual_seed(3)
    with torch.no_grad():
        b = twin(d, c)[1]
    assert torch.equal(a, b) and b.grad_fn is None


def test_default_constructor_still_refuses_train_mode_and_flags_add_no_parameter():
    plain = T.build_model({})
    flagged = T.build_model({}, trainable=True, sparse_grad=True)
    sa, sb = plain.state_dict(), flagged.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    dense, cat = T.model_inputs(17)
    with pytest.raises(NotImplementedError):
        plain.to(DEV).train()(dense.to(DEV), H.to_device(cat, DEV))


def test_empty_batch_in_train_mode_gives_empty_outputs_and_zero_gradients():
    model = T.build_model({}, trainable=True).to(DEV).train()
    dense, cat = T.model_inputs(17)
    d0, c0 = dense[:0].to(DEV), {k: v[:0].to(DEV) for k, v in cat.items()}
    K = len(model.task_names)
    probs, logits = model(d0, c0)
    assert probs.shape == (0, K) and logits.shape == (0, K) and logits.requires_grad
    rankops.esmm_loss(logits, torch.zeros(0, K, device=DEV)).backward()
    assert all(p.grad is not None and bool((p.grad == 0).all()) for p in model.parameters())
    with torch.no_grad():
        q = model(d0, c0)
    assert q[0].shape == (0, K) and q[1].grad_fn is None and rankops.error_flags() == 0


def test_sparse_grad_equals_dense_and_sparse_adam_steps():
    B = 300
    dense, cat = T.model_inputs(B)
    d, c = dense.to(DEV), H.to_device(cat, DEV)
    grads = []
    for sparse in (False, True):
        model = T.build_model({}, trainable=True, sparse_grad=sparse).to(DEV).train()
        torch.manual_seed(5)
        model_loss(*model(d, c)).backward()
        grads.append({n: p.grad for n, p in model.named_parameters() if p.grad is not None})
    for n, g in grads[0].items():
        s = grads[1][n]
        if is_table(n):
            # same dx rows; the dense path adds duplicate ids with float atomics, to_dense() coalesces in index
            # order: the sums differ in rounding only, so the drift tolerance of the tables, not bits
            assert s.is_sparse
            close(s.to_dense(), g.cpu().double(), T.DX_TOL, f"sparse {n}")
        else:
            assert torch.equal(s, g), n
    tables = [p for n, p in model.named_parameters() if is_table(n) and p.grad is not None]
    rest = [p for n, p in model.named_parameters() if not is_table(n)]
    before = rest[0].detach().clone()
    rankops.SparseAdam(tables, lr=1e-3).step()
    rankops.Adam(rest, lr=1e-3).step()
    torch.cuda.synchronize()
    assert not torch.equal(before, rest[0].detach()) and rankops.error_flags() == 0


def test_captured_step_replays_follow_the_optimizer_then_eval_and_prepare_see_the_weights():
    B, lr = 64, 1e-3
    a = T.build_model({}, trainable=True).to(DEV).train()
    b = T.build_model({}, trainable=True).to(DEV).train()
    oa = rankops.Adam(a.parameters(), lr=lr, capturable=True)
    ob = rankops.Adam(b.parameters(), lr=lr, capturable=True)
    dense, cat = T.model_inputs(B)
    d, c = dense.to(DEV), H.to_device(cat, DEV)
    K = len(a.task_names)
    y = (torch.rand(B, K, generator=torch.Generator().manual_seed(4)) < 0.5).float()
    labels = torch.cumprod(y, dim=1).to(DEV)

    def step(model, opt):
        opt.zero_grad(set_to_none=True)
        rankops.esmm_loss(model(d, c)[1], labels).backward()
        opt.step()

    torch.manual_seed(9)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(a, oa)                      # warm-up: step 1 (stream counter 1)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    oa.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        step(a, oa)                      # captured, not run
    torch.manual_seed(9)
    step(b, ob)
    for i in range(3):                   # three replays against three eager steps, the same masks by the counter
        graph.replay()
        step(b, ob)
        torch.cuda.synchronize()
        for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
            _assert_adam_params_close(pa.detach().cpu(), pb.detach().cpu(), lr=lr, steps=i + 2, what=f"{n} after replay {i}")
    fresh = T.build_model({})
    assert not torch.equal(fresh.towers[0][0].weight, a.towers[0][0].weight.cpu())
    # eval and prepare() after the steps read the stepped weights
    a.eval()
    ref = R.forward(R.floats(H.cpu_params(a), torch.float64), dense, cat)
    with torch.no_grad():
        probs, logits = a(d, c)
        pp, pl = a.prepare(d, c)()
    close(logits, ref[1], R.LOGIT_TOL, "eval logits after training")
    close(probs, ref[0], R.PROB_TOL, "eval probs after training")
    assert torch.equal(pp, probs) and torch.equal(pl, logits)
    assert rankops.error_flags() == 0
