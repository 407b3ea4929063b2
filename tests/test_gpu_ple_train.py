"""PLE training on the GPU: differentiable rankops.ple, the two new entry points' envelopes and
PLE(trainable=True), against the float64 autograd restatement (tests/ple_train_ref.py, which states the
tolerances and where they come from)."""
import ctypes

import pytest
import torch

import helpers as H
import ple_ref as R
import ple_train_ref as T
import rankops
from launch_count import launches_of
from rankops import _lib, ops
from test_gpu_train import _assert_adam_params_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.0
INVALID = 1  # RK_ERR_INVALID (include/rankops.h)
CASE_IDS = [c[0] for c in T.GRAD_CASES]


def close(got, ref, tol, what):
    err = R.rel_err(got, ref)
    print(f"{what}: rel err {err:.3e} (tolerance {tol:.1e})")
    assert got.shape == ref.shape and err <= tol, f"{what}: {err:.3e} > {tol:.1e}"


def to_gpu(obj, grad):
    if obj is None:
        return None
    if isinstance(obj, torch.Tensor):
        return obj.to(DEV).requires_grad_(grad)
    return type(obj)(to_gpu(o, grad) for o in obj)


def no_biases(levels, towers):
    nb = lambda layers: [(w, None) for w, _ in layers]  # noqa: E731
    levels = [([[nb(e) for e in task] for task in sp], [nb(e) for e in sh], nb(gt), None if sg is None else (sg[0], None))
              for sp, sh, gt, sg in levels]
    return levels, [(nb(hidden), out) for hidden, out in towers]


def run_op(c, pad=R.ROW_PAD, with_towers=True, bias=True):
    """Differentiable rankops.ple on one case (with towers the loss over logits and probs, without over the
    last level's representations); returns T.op_gradients' dict of GPU results."""
    rows, levels, towers = T.op_inputs(c)
    width = c[1]
    if not bias:
        levels, towers = no_biases(levels, towers)
    xb = rows[:, :width + pad].contiguous().to(DEV).requires_grad_(True)
    gl, gt = to_gpu(levels, True), to_gpu(towers if with_towers else None, True)
    out = rankops.ple(xb[:, :width], gl, gt)
    assert all(o.grad_fn is not None for o in out)
    B, K, Hh = c[8], c[3], c[6][-1]
    cm, cl, cp = (t.float().to(DEV) for t in T.loss_coeffs(B, K, Hh))
    loss = (cl * out[0]).sum() + (cp * out[1]).sum() if with_towers else (cm * out[0]).sum()
    loss.backward()
    grads = lambda ts: [t.grad if t.grad is not None else torch.zeros_like(t) for t in ts]  # noqa: E731
    stacks, gates = T.split_levels(gl)
    return dict(out=tuple(o.detach() for o in out), dx=xb.grad[:, :width], pad=xb.grad[:, width:], experts=grads(stacks),
                gates=grads(gates), towers=grads(T.flat(gt)))


def compare(got, ref, name, what="", tols=None):
    """Every gradient against the restatement; all figures are printed before the first failure is raised."""
    dx, dw, dgate = tols or T.tolerances(name)
    assert len(got["experts"]) == len(ref["experts"]) and len(got["towers"]) == len(ref["towers"])
    assert len(got["gates"]) == len(ref["gates"])
    items = [(got["dx"], ref["dx"], dx, "dx")]
    items += [(a, b, dw, f"tower grad {i}") for i, (a, b) in enumerate(zip(got["towers"], ref["towers"]))]
    items += [(a, b, dw, f"expert grad {i}") for i, (a, b) in enumerate(zip(got["experts"], ref["experts"]))]
    items += [(a, b, dgate, f"gate grad {i}") for i, (a, b) in enumerate(zip(got["gates"], ref["gates"]))]
    bad, worst = [], [0.0, 0.0, 0.0]
    for a, b, tol, what_ in items:
        err = R.rel_err(a, b)
        g = 0 if what_ == "dx" else 2 if what_.startswith("gate") else 1
        worst[g] = max(worst[g], err)
        if a.shape != b.shape or not err <= tol:
            bad.append(f"{what_}: {err:.3e} > {tol:.1e}")
    print(f"{name}{what}: worst rel err dx {worst[0]:.3e} ({dx:.1e}), dw {worst[1]:.3e} ({dw:.1e}), "
          f"dgate {worst[2]:.3e} ({dgate:.1e})")
    assert not bad, f"{name}{what}: " + "; ".join(bad)


def same_bits(a, b, what):
    for key in ("dx", "experts", "gates", "towers"):
        xs, ys = (a[key], b[key]) if isinstance(a[key], list) else ([a[key]], [b[key]])
        assert len(xs) == len(ys) and all(torch.equal(x, y) for x, y in zip(xs, ys)), f"{what}: {key} differs"


# ---------------------------------------------------------------- op level

@pytest.mark.parametrize("c", T.GRAD_CASES, ids=CASE_IDS)
def test_op_gradients_match_restatement(c):
    name = c[0]
    ref = T.op_reference(c)
    got = run_op(c)
    _, _, lt, pt = R.tolerances(name)
    close(got["out"][0], ref["out"][1], lt, f"{name} logits")
    close(got["out"][1], ref["out"][2], pt, f"{name} probs")
    compare(got, ref, name)
    assert bool((got["pad"] == 0).all())  # the pad columns of the row buffer take no gradient
    same_bits(got, run_op(c), f"{name} repeat")                 # no atomics, fixed-order sums
    same_bits(got, run_op(c, pad=0), f"{name} rows without padding")
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("name", ["tile_edge", "odd", "deep", "many"])
def test_op_without_towers_takes_the_gradient_of_the_last_representations(name):
    c = T.case(name)
    ref = T.op_reference(c, towers=False)
    got = run_op(c, with_towers=False)
    rt, gt, _, _ = R.tolerances(name)
    close(got["out"][0], ref["out"][0][-1][0], rt, f"{name} last representations")
    close(got["out"][1], ref["out"][0][-1][1], gt, f"{name} last task gates")
    compare(got, ref, name, " (towers None)")
    assert rankops.error_flags() == 0


def test_one_level_without_task_experts_has_mmoes_gradients():
    c = T.case("mmoe_like")
    rows, levels, towers = T.op_inputs(c)
    (_, experts, gates, _), = levels
    x = rows[:, :c[1]].contiguous().to(DEV).requires_grad_(True)
    ge, gg, gt = to_gpu(experts, True), to_gpu(gates, True), to_gpu(towers, True)
    _, _, logits, probs = rankops.mmoe(x, ge, gg, gt)
    _, cl, cp = (t.float().to(DEV) for t in T.loss_coeffs(c[8], c[3], c[6][-1]))
    ((cl * logits).sum() + (cp * probs).sum()).backward()
    mm = dict(dx=x.grad.double().cpu(), experts=[t.grad.double().cpu() for t in T.flat(ge)],
              gates=[t.grad.double().cpu() for t in T.flat(gg)], towers=[t.grad.double().cpu() for t in T.flat(gt)])
    compare(run_op(c, pad=0), mm, "mmoe_like", " (against rankops.mmoe)")


def test_op_without_grad_is_the_eval_launch_and_p0_train_forward_has_its_bits():
    c = T.case("odd")  # three levels, widths off the 4 grid
    rows, levels, towers = T.op_inputs(c)
    x = rows[:, :c[1]].to(DEV)
    plain = rankops.ple(x, to_gpu(levels, False), to_gpu(towers, False), return_levels=True)
    with torch.no_grad():
        quiet = rankops.ple(x, to_gpu(levels, True), to_gpu(towers, True), return_levels=True)
    tracked = rankops.ple(x, to_gpu(levels, True), to_gpu(towers, True), return_levels=True)
    assert plain[0].grad_fn is None and quiet[0].grad_fn is None and tracked[0].grad_fn is not None
    for other in (quiet, tracked):
        assert torch.equal(plain[0], other[0]) and torch.equal(plain[1], other[1])
        for a, b in zip(plain[2], other[2]):  # every level's representations and gates
            assert all((s is None and t is None) or torch.equal(s, t) for s, t in zip(a, b))
    assert rankops.error_flags() == 0


def test_refusals_missing_biases_and_the_empty_batch():
    c = T.case("odd")
    rows, levels, towers = T.op_inputs(c)
    x = rows[:, :c[1]].to(DEV)
    gl = to_gpu(levels, True)
    logits, probs, lv = rankops.ple(x, gl, to_gpu(towers, True), return_levels=True)
    with pytest.raises(NotImplementedError, match="gate output"):
        lv[-1][1].sum().backward(retain_graph=True)        # a task gate of the last level
    with pytest.raises(NotImplementedError, match="gate output"):
        lv[0][2].sum().backward(retain_graph=True)         # a shared gate
    with pytest.raises(NotImplementedError, match="lower level"):
        lv[0][0].sum().backward(retain_graph=True)         # a lower level's representations
    # bias=None everywhere but the output layers: no bias gradient, the others unchanged in meaning
    nl, nt = no_biases(levels, towers)
    ref = T.op_gradients(rows[:, :c[1]], nl, nt)
    got = run_op(c, bias=False)
    assert len(got["experts"]) == c[2] * (c[3] * c[4] + c[5]) * len(c[6])
    compare(got, ref, "odd", " (no biases)")
    x0 = torch.zeros(0, c[1], device=DEV, requires_grad=True)
    l0, p0 = rankops.ple(x0, gl, to_gpu(towers, True))
    assert l0.shape == (0, c[3]) and p0.shape == (0, c[3])
    (l0.sum() + p0.sum()).backward()
    assert x0.grad.shape == (0, c[1]) and all(bool((w.grad == 0).all()) for w in T.split_levels(gl)[0])
    assert rankops.error_flags() == 0


# ---------------------------------------------------------------- raw ABI

def _i32(values):
    return (ctypes.c_int32 * len(values))(*values)


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t if isinstance(t, int) or t is None else t.data_ptr() for t in ts])


def test_mix_backward_one_column_gates_and_envelope():
    lib = _lib.load()
    _lib.ensure_device(torch.device(DEV))
    st = _lib.raw_stream(DEV)
    B, K, Hh = 5, 2, 8     # ms = 0, mc = 1: one-column task gates, the last level (no shared mixture)
    g = torch.Generator().manual_seed(3)
    dm = torch.randn(B, K * Hh, generator=g).to(DEV)
    f = torch.randn(B, Hh, generator=g).to(DEV)
    gates = torch.ones(B, K, device=DEV)
    dgl, dz = torch.full((B, 2 * 4), SENTINEL, device=DEV), torch.full((B, Hh), SENTINEL, device=DEV)

    def mix(K=K, ms=0, mc=1, Hh=Hh, dm_=dm.data_ptr(), dz_=dz.data_ptr(), goff=(0, 4), soff=None, B=B):
        soff = soff or [0] * (K * ms + mc)
        return lib.rk_ple_mix_backward(B, K, ms, mc, 0, Hh, dm_, dm.shape[1], 8, f.data_ptr(), f.shape[1], 8, gates.data_ptr(),
                                       gates.shape[1], 2.0, dgl.data_ptr(), dgl.shape[1], _i32(list(goff) + [0] * 9),
                                       dz_, dz.shape[1], _i32(list(soff)), 8, st)
    assert mix(dm_=None) == INVALID and "rk_ple_mix_backward" in _lib.last_error()
    assert mix(K=9) == _lib.RK_ERR_UNSUPPORTED          # tasks
    assert mix(K=1, mc=65) == _lib.RK_ERR_UNSUPPORTED   # stacks
    assert mix(Hh=513) == _lib.RK_ERR_UNSUPPORTED
    assert mix(dz_=dz.data_ptr() + 2) == INVALID        # misaligned
    assert mix(goff=(0, 8)) == INVALID                  # a gate's columns past the row
    assert mix(soff=[4]) == INVALID                     # a stack's columns past the row
    assert mix(B=-1) == INVALID
    torch.cuda.synchronize()
    assert bool((dgl == SENTINEL).all()) and bool((dz == SENTINEL).all())
    assert mix(B=0) == _lib.RK_OK
    torch.cuda.synchronize()
    assert bool((dgl == SENTINEL).all()) and bool((dz == SENTINEL).all())
    assert mix() == _lib.RK_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert bool((dgl == 0).all())  # softmax over one column: exactly zero, pad columns included
    want = (dm[:, :Hh] + dm[:, Hh:]) * 2.0 * (f > 0)
    assert torch.allclose(dz, want, rtol=1e-6, atol=1e-6)
    again = torch.full_like(dz, SENTINEL)
    assert mix(dz_=again.data_ptr()) == _lib.RK_OK and torch.equal(again, dz)
    assert rankops.error_flags() == 0


def test_train_forward_envelope():
    lib = _lib.load()
    dev = torch.device(DEV)
    _lib.ensure_device(dev)
    width, L, K, ms, mc, n = 20, 2, 2, 1, 1, 16
    NE, GT = K * ms + mc, ms + mc
    img = torch.zeros(64, 64, device=DEV)
    x = torch.ones(4, width, device=DEV)
    full = lambda *shape: torch.full(shape, SENTINEL, device=DEV)  # noqa: E731
    xo, ea = full(4, width), [full(4, NE * n) for _ in range(L)]
    reps = [full(4, (K + (j < L - 1)) * n) for j in range(L)]
    gates = [full(4, K * GT + (NE if j < L - 1 else 0)) for j in range(L)]

    def call(p=0.0, xo_=xo, ea_=None, K=K, ms=ms, mc=mc, n=n, reps_=None):
        entries = [(img, None)] * (L * (K * ms + mc) + L * (K + 1))
        args, keep = ops.ple_forward_args([ops.dense_segment(x, width, 0)], width, 4, L, K, ms, mc, [n], [], entries, False, dev)
        return lib.rk_ple_forward_train(*args[:15], p, 0, None, ops.ptr(xo_) if isinstance(xo_, torch.Tensor) else xo_,
                                        _ptrs(ea_ or ea), None, None, None, _ptrs(reps_ or reps), _ptrs(gates),
                                        _lib.raw_stream(dev))
    assert call(xo_=None) == INVALID and "rk_ple_forward_train" in _lib.last_error()
    assert call(reps_=[reps[0], None]) == INVALID
    assert call(p=0.5) == INVALID          # dropout without a stream slot
    assert call(p=1.0) == INVALID
    assert call(ea_=[ea[0], ea[1].data_ptr() + 4]) == INVALID
    assert call(K=9, ms=0) == _lib.RK_ERR_UNSUPPORTED
    assert call(K=1, ms=0, mc=65) == _lib.RK_ERR_UNSUPPORTED
    assert call(n=513) == _lib.RK_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in [xo] + ea + reps + gates)
    assert call() == _lib.RK_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert bool((xo == 1).all()) and all(bool((t == 0).all()) for t in ea + reps)
    assert bool((gates[1] == 0.5).all()) and bool((gates[0][:, :K * GT] == 0.5).all())
    assert rankops.error_flags() == 0


# ---------------------------------------------------------------- the model

def engine_keeps(model, B):
    """The dropout multipliers the last train forward drew, by the documented site numbering."""
    slot = model._dropout.counter - 1
    return {s: ops.dropout_mask(model._dropout.seed + s, slot, B, n, model.dropout_rate).cpu().double()
            for s, n in T.model_sites(model)}


def model_loss(probs, logits):
    B, K = logits.shape
    _, cl, cp = (t.float().to(logits.device) for t in T.loss_coeffs(B, K, 1))
    return (cl * logits).sum() + (cp * probs).sum()


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
    tol = (T.DX_TOL, T.DW_TOL, T.DGATE_TOL)
    worst, bad = [0.0, 0.0, 0.0], []
    for name, prm in model.named_parameters():
        assert prm.grad is not None and prm.grad.shape == ref[name].shape, name
        err, g = R.rel_err(prm.grad, ref[name]), T.group_of(name)
        worst[g] = max(worst[g], err)
        if not err <= tol[g]:
            bad.append(f"{name}: {err:.3e} > {tol[g]:.1e}")
    print(f"{mc[0]}: worst rel err tables {worst[0]:.3e}, dw {worst[1]:.3e}, dgate {worst[2]:.3e}")
    assert not bad, "; ".join(bad)
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
    assert tp.grad_fn is not None and torch.equal(tp.detach(), ep) and torch.equal(tl.detach(), el)
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
    assert torch.equal(a, b) and b.grad_fn is None and not torch.equal(a, el)


def test_empty_batch_in_train_mode_gives_empty_outputs_and_zero_gradients():
    model = T.build_model({}, trainable=True).to(DEV).train()
    dense, cat = T.model_inputs(17)
    d0, c0 = dense[:0].to(DEV), {k: v[:0].to(DEV) for k, v in cat.items()}
    K = len(model.task_names)
    probs, logits = model(d0, c0)
    assert probs.shape == (0, K) and logits.shape == (0, K) and logits.requires_grad
    torch.nn.BCEWithLogitsLoss(reduction="sum")(logits, torch.zeros(0, K, device=DEV)).backward()
    assert all(p.grad is not None and bool((p.grad == 0).all()) for p in model.parameters())
    with torch.no_grad():
        q = model(d0, c0)
    assert q[0].shape == (0, K) and q[1].grad_fn is None and rankops.error_flags() == 0


def test_sparse_grad_equals_dense_and_sparse_adam_steps():
    B = 300
    dense, cat = T.model_inputs(B)
    d, c = dense.to(DEV), H.to_device(cat, DEV)
    grads, models = [], []
    for sparse in (False, True):
        model = T.build_model({}, trainable=True, sparse_grad=sparse).to(DEV).train()
        torch.manual_seed(5)
        model_loss(*model(d, c)).backward()
        grads.append({n: p.grad for n, p in model.named_parameters() if p.grad is not None})
        models.append(model)
    for n, g in grads[0].items():
        s = grads[1][n]
        if is_table(n):
            # same dx rows; the dense path adds duplicate ids with float atomics, to_dense() coalesces in index
            # order: the sums differ in rounding only, so the drift tolerance of the tables, not bits
            assert s.is_sparse
            close(s.to_dense(), g.cpu().double(), T.DX_TOL, f"sparse {n}")
        else:
            assert torch.equal(s, g), n
    lr = 1e-3
    for model, Opt in zip(models, (rankops.Adam, rankops.SparseAdam)):
        tables = [p for n, p in model.named_parameters() if is_table(n) and p.grad is not None]
        Opt(tables, lr=lr).step()
    torch.cuda.synchronize()
    fresh = T.build_model({})
    # Adam's first step moves an element by lr g / (|g| + eps), about lr sign(g) (and a row that was not looked
    # up, g = 0, not at all, lazily or not).  The two gradients agree within DX_TOL (1 + |g|) < 2e-4, so where
    # |g| >= 1e-3 they have one sign and the steps agree to rounding; below that the sign may differ and the
    # steps lie at most 2 lr apart.
    for n, p in models[0].named_parameters():
        if is_table(n) and p.grad is not None:
            q, g = dict(models[1].named_parameters())[n].detach().cpu(), grads[0][n].cpu()
            p = p.detach().cpu()
            assert not torch.equal(p, dict(fresh.named_parameters())[n].detach())
            diff, sure = (q - p).abs(), g.abs() >= 1e-3
            print(f"{n}: {int(sure.sum())} elements with |g| >= 1e-3 differ by at most {float(diff[sure].max()):.2e}, "
                  f"the other {int((~sure).sum())} by at most {float(diff[~sure].max()):.2e}")
            assert bool(sure.any()) and float(diff[sure].max()) <= 1e-6 and float(diff.max()) <= 2 * lr * (1 + 1e-3)
    assert rankops.error_flags() == 0


def test_captured_step_replays_follow_the_optimizer_then_eval_and_prepare_see_the_weights():
    B, lr = 64, 1e-3
    a = T.build_model({}, trainable=True).to(DEV).train()
    b = T.build_model({}, trainable=True).to(DEV).train()
    oa = rankops.Adam(a.parameters(), lr=lr, capturable=True)
    ob = rankops.Adam(b.parameters(), lr=lr, capturable=True)
    dense, cat = T.model_inputs(B)
    d, c = dense.to(DEV), H.to_device(cat, DEV)
    K = len(a.task_names)
    labels = (torch.rand(B, K, generator=torch.Generator().manual_seed(4)) < 0.3).float().to(DEV)
    crit = torch.nn.BCEWithLogitsLoss()

    def step(model, opt):
        opt.zero_grad(set_to_none=True)
        crit(model(d, c)[1], labels).backward()
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
    assert not torch.equal(fresh.levels[1].shared_experts[0][0].weight, a.levels[1].shared_experts[0][0].weight.cpu())
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


def test_launch_list_does_not_depend_on_tasks_or_experts():
    dense, cat = T.model_inputs(64)
    d, c = dense.to(DEV), H.to_device(cat, DEV)
    lists = []
    for K, ms, mc in ((2, 1, 1), (3, 2, 2)):
        kw = dict(num_levels=2, num_specific_experts=ms, num_shared_experts=mc, expert_hidden_units=(32, 16),
                  tower_hidden_units=(8,), task_names=("read_comment", "like", "click_avatar")[:K])
        model = T.build_model(kw, trainable=True).to(DEV).train()

        def step():
            model.zero_grad(set_to_none=True)
            probs, logits = model(d, c)
            model_loss(probs, logits).backward()
        step()
        lists.append(launches_of(step))
    assert lists[0] == lists[1], (lists[0], lists[1])
    names = lists[0]
    assert names.count("rk_ple_forward_train") == 1 and names.count("rk_ple_mix_backward") == 2
    assert names.count("rk_mmoe_head_backward") == 1 and names.count("rk_mlp_pack_weights") == 1
    print(f"{len(names)} launches: {names}")
