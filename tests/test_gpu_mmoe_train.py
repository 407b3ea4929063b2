"""MMoE training on the GPU: differentiable rankops.mmoe, the new entry points' envelopes and
MMoE(trainable=True), against the float64 autograd restatement (tests/mmoe_train_ref.py, which states the
tolerances and where they come from)."""
import ctypes

import pytest
import torch

import helpers as H
import mmoe_ref as R
import mmoe_train_ref as T
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
    assert got.shape == ref.shape and err <= tol, f"{what}: {err:.3e} > {tol:.1e}"


def to_gpu(obj, grad):
    if obj is None:
        return None
    if isinstance(obj, torch.Tensor):
        return obj.to(DEV).requires_grad_(grad)
    return type(obj)(to_gpu(o, grad) for o in obj)


def run_op(c, pad=R.ROW_PAD, use=("mixed", "logits", "probs"), with_towers=True, bias=True):
    """Differentiable rankops.mmoe on one case; returns T.op_gradients' dict of GPU results."""
    rows, experts, gates, towers = T.op_inputs(c)
    width = c[1]
    if not bias:
        experts = [[(w, None) for w, _ in layers] for layers in experts]
        gates = [(w, None) for w, _ in gates]
        towers = [([(w, None) for w, _ in hidden], out) for hidden, out in towers]
    xb = rows[:, :width + pad].contiguous().to(DEV).requires_grad_(True)
    ge, gg, gt = to_gpu(experts, True), to_gpu(gates, True), to_gpu(towers if with_towers else None, True)
    out = rankops.mmoe(xb[:, :width], ge, gg, gt)
    assert all(o.grad_fn is not None for o in out)
    B, K, Hh = out[0].shape
    cm, cl, cp = (t.float().to(DEV) for t in T.loss_coeffs(B, K, Hh))
    loss = torch.zeros((), device=DEV)
    if "mixed" in use:
        loss = loss + (cm * out[0]).sum()
    if with_towers and "logits" in use:
        loss = loss + (cl * out[2]).sum()
    if with_towers and "probs" in use:
        loss = loss + (cp * out[3]).sum()
    loss.backward()
    grads = lambda ts: [t.grad if t.grad is not None else torch.zeros_like(t) for t in ts]  # noqa: E731
    return dict(out=tuple(o.detach() for o in out), dx=xb.grad[:, :width], pad=xb.grad[:, width:], experts=grads(T.flat(ge)),
                gates=grads(T.flat(gg)), towers=grads(T.flat(gt)))


def compare(got, ref, name, what=""):
    """Every gradient against the restatement; all figures are printed before the first failure is raised."""
    dx, dw, dgate = T.tolerances(name)
    assert len(got["experts"]) == len(ref["experts"]) and len(got["towers"]) == len(ref["towers"])
    items = [(got["dx"], ref["dx"], dx, "dx")]
    items += [(a, b, dw, f"tower grad {i}") for i, (a, b) in enumerate(zip(got["towers"], ref["towers"]))]
    items += [(a, b, dw, f"expert grad {i}") for i, (a, b) in enumerate(zip(got["experts"], ref["experts"]))]
    items += [(a, b, dgate, f"gate grad {i}") for i, (a, b) in enumerate(zip(got["gates"], ref["gates"]))]
    bad = []
    for a, b, tol, what_ in items:
        err = R.rel_err(a, b)
        print(f"{name}{what} {what_}: rel err {err:.3e} (tolerance {tol:.1e})")
        if a.shape != b.shape or not err <= tol:
            bad.append(f"{what_}: {err:.3e} > {tol:.1e}")
    assert not bad, f"{name}{what}: " + "; ".join(bad)


def same_bits(a, b, what):
    for key in ("dx", "experts", "gates", "towers"):
        xs, ys = (a[key], b[key]) if isinstance(a[key], list) else ([a[key]], [b[key]])
        assert len(xs) == len(ys) and all(torch.equal(x, y) for x, y in zip(xs, ys)), f"{what}: {key} differs"


# ---------------------------------------------------------------- op level

@pytest.mark.parametrize("c", T.GRAD_CASES, ids=[c[0] for c in T.GRAD_CASES])
def test_op_gradients_match_restatement(c):
    ref = T.op_reference(c)
    got = run_op(c)
    mt, gt, lt, pt = R.tolerances(c[0])
    for o, r, t, n in zip(got["out"], ref["out"], (mt, gt, lt, pt), ("mixed", "gates", "logits", "probs")):
        close(o, r, t, f"{c[0]} {n}")
    compare(got, ref, c[0])
    assert bool((got["pad"] == 0).all())  # the pad columns of the row buffer take no gradient
    same_bits(got, run_op(c), f"{c[0]} repeat")                 # no atomics, fixed-order sums
    same_bits(got, run_op(c, pad=0), f"{c[0]} rows without padding")
    if c[0] == "one_expert":  # softmax over one expert: the gate gradients are exactly zero
        assert all(bool((g == 0).all()) for g in got["gates"])
    assert rankops.error_flags() == 0


def test_op_without_grad_is_the_eval_launch():
    c = R.case("tile_edge")
    rows, experts, gates, towers = T.op_inputs(c)
    x = rows[:, :c[1]].to(DEV)
    plain = rankops.mmoe(x, to_gpu(experts, False), to_gpu(gates, False), to_gpu(towers, False))
    assert all(o.grad_fn is None and not o.requires_grad for o in plain)
    tracked = run_op(c)["out"]
    with torch.no_grad():
        quiet = rankops.mmoe(x, to_gpu(experts, True), to_gpu(gates, True), to_gpu(towers, True))
    assert all(o.grad_fn is None for o in quiet)
    for a, b, q in zip(plain, tracked, quiet):  # the train forward without dropout has the eval kernel's bits
        assert torch.equal(a, b) and torch.equal(a, q)


@pytest.mark.parametrize("name", ["odd", "deep"])
def test_op_single_outputs_and_missing_biases(name):
    c = T.case(name)
    rows, experts, gates, towers = T.op_inputs(c)
    x = rows[:, :c[1]]
    # dmixed alone, no towers at all
    ref = T.op_gradients(x, experts, gates, None, use=("mixed",))
    compare(run_op(c, use=("mixed",), with_towers=False), ref, name, " (towers None)")
    # dlogits alone
    ref = T.op_gradients(x, experts, gates, towers, use=("logits",))
    compare(run_op(c, use=("logits",)), ref, name, " (dlogits)")
    # bias=None everywhere but the output layers: no bias gradient, the others unchanged in meaning
    nb_e = [[(w, None) for w, _ in layers] for layers in experts]
    nb_g = [(w, None) for w, _ in gates]
    nb_t = [([(w, None) for w, _ in hidden], out) for hidden, out in towers]
    ref = T.op_gradients(x, nb_e, nb_g, nb_t)
    got = run_op(c, bias=False)
    assert len(got["experts"]) == c[2] * len(c[4]) and len(got["gates"]) == c[3]
    compare(got, ref, name, " (no biases)")
    assert rankops.error_flags() == 0


def test_op_gate_probs_gradient_is_refused_and_empty_batch():
    c = R.case("tile_edge")
    rows, experts, gates, towers = T.op_inputs(c)
    ge = to_gpu(experts, True)
    out = rankops.mmoe(rows[:, :c[1]].to(DEV), ge, to_gpu(gates, True), to_gpu(towers, True))
    with pytest.raises(NotImplementedError, match="gate_probs"):
        out[1].sum().backward()
    x0 = torch.zeros(0, c[1], device=DEV, requires_grad=True)
    out = rankops.mmoe(x0, ge, to_gpu(gates, True), to_gpu(towers, True))
    assert out[0].shape == (0, c[3], c[4][-1]) and out[2].shape == (0, c[3])
    (out[0].sum() + out[3].sum()).backward()
    assert x0.grad.shape == (0, c[1]) and all(bool((w.grad == 0).all()) for w in T.flat(ge))


# ---------------------------------------------------------------- raw ABI envelopes

def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t if isinstance(t, int) else t.data_ptr() for t in ts])


def test_grouped_gemm_envelopes():
    lib = _lib.load()
    _lib.ensure_device(torch.device(DEV))
    st = _lib.raw_stream(DEV)
    M, N, Rr, G = 8, 8, 8, 2
    A = [torch.ones(M, Rr, device=DEV) for _ in range(17)]
    Bm = [torch.ones(N, Rr, device=DEV) for _ in range(17)]
    C = [torch.full((M, N), SENTINEL, device=DEV) for _ in range(17)]

    def call(G=G, a=None, c=None):
        return lib.rk_gemm_grouped(G, 0, 0, M, N, Rr, _ptrs(a or A[:G]), Rr, _ptrs(Bm[:G]), Rr, _ptrs(c or C[:G]), N, None,
                                   0, 1.0, 0, st)
    assert call(a=[A[0], 0]) == INVALID and "rk_gemm_grouped" in _lib.last_error()      # a null operand
    assert call(G=17) == _lib.RK_ERR_UNSUPPORTED                                                      # G above the limit
    assert call(c=[C[0], C[1].data_ptr() + 2]) == INVALID                                 # misaligned
    torch.cuda.synchronize()
    assert all(bool((c == SENTINEL).all()) for c in C)
    assert call() == _lib.RK_OK
    assert bool((C[0] == Rr).all()) and bool((C[1] == Rr).all()) and bool((C[2] == SENTINEL).all())

    W = [torch.full((8, 8), SENTINEL, device=DEV) for _ in range(17)]
    db = [torch.full((8,), SENTINEL, device=DEV) for _ in range(17)]
    nws = lib.rk_gemm_wgrad_grouped_workspace_floats(17, 8, 8, M)
    ws = torch.empty(max(nws, 1 << 16), device=DEV)

    def wcall(G=G, a=None, c=None):
        return lib.rk_gemm_wgrad_grouped(G, 8, 8, M, _ptrs(a or A[:G]), Rr, _ptrs(Bm[:G]), Rr, _ptrs(c or W[:G]), 8,
                                         _ptrs(db[:G]), 0, ws.data_ptr(), ws.numel(), st)
    assert wcall(a=[A[0], 0]) == INVALID and "rk_gemm_wgrad_grouped" in _lib.last_error()
    assert wcall(G=17) == _lib.RK_ERR_UNSUPPORTED
    assert wcall(c=[W[0], W[1].data_ptr() + 4]) == _lib.RK_ERR_UNSUPPORTED  # not 16-B aligned: as rk_gemm_wgrad
    torch.cuda.synchronize()
    assert all(bool((w == SENTINEL).all()) for w in W) and all(bool((b == SENTINEL).all()) for b in db)
    assert wcall() == _lib.RK_OK
    assert bool((W[0] == M).all()) and bool((db[1] == M).all()) and bool((W[2] == SENTINEL).all())


def test_pack_weights_envelope():
    lib = _lib.load()
    _lib.ensure_device(torch.device(DEV))
    st = _lib.raw_stream(DEV)
    w = torch.arange(12.0, device=DEV).view(3, 4)
    img = torch.full((2, 64, 64), SENTINEL, device=DEV)

    def call(items):
        arr = (_lib.PackItem * len(items))()
        for it, (wp, out, ldw, n, k) in zip(arr, items):
            it.w, it.out, it.ldw, it.n, it.k = wp, out, ldw, n, k
        return lib.rk_mlp_pack_weights(arr, len(items), st)
    good = (w.data_ptr(), img[0].data_ptr(), 4, 3, 4)
    assert lib.rk_mlp_pack_weights(None, 1, st) == INVALID and "rk_mlp_pack_weights" in _lib.last_error()
    assert call([good, (None, img[1].data_ptr(), 4, 3, 4)]) == INVALID            # a null weight
    assert call([good, (w.data_ptr(), img[1].data_ptr() + 4, 4, 3, 4)]) == INVALID  # image not 16-B aligned
    assert call([good, (w.data_ptr(), img[1].data_ptr(), 3, 3, 4)]) == INVALID      # ldw < k
    torch.cuda.synchronize()
    assert bool((img == SENTINEL).all())   # a bad item anywhere: nothing is written, the good item included
    assert call([good, (w.data_ptr(), img[1].data_ptr(), 4, 3, 4)]) == _lib.RK_OK
    assert torch.equal(img[0], ops.pack_mlp_weight(w)) and torch.equal(img[1], img[0])
    assert lib.rk_mlp_pack_weights(None, 0, st) == _lib.RK_OK


def test_mix_and_head_backward_envelopes():
    lib = _lib.load()
    _lib.ensure_device(torch.device(DEV))
    st = _lib.raw_stream(DEV)
    B, E, K, Hh = 4, 2, 2, 8
    dm, f, g = torch.ones(B, K * Hh, device=DEV), torch.ones(B, E * Hh, device=DEV), torch.full((B, K, E), 0.5, device=DEV)
    dgl, dz = torch.full((B, K * E), SENTINEL, device=DEV), torch.full((B, E * Hh), SENTINEL, device=DEV)

    def mix(E=E, K=K, dm_=dm.data_ptr(), dz_=dz.data_ptr()):
        return lib.rk_mmoe_mix_backward(B, E, K, Hh, dm_, K * Hh, Hh, f.data_ptr(), E * Hh, Hh, g.data_ptr(), 1.0,
                                        dgl.data_ptr(), K * E, dz_, E * Hh, Hh, st)
    assert mix(dm_=None) == INVALID and "rk_mmoe_mix_backward" in _lib.last_error()
    assert mix(E=17, K=1) == _lib.RK_ERR_UNSUPPORTED
    assert mix(dz_=dz.data_ptr() + 2) == INVALID
    torch.cuda.synchronize()
    assert bool((dgl == SENTINEL).all()) and bool((dz == SENTINEL).all())
    assert mix() == _lib.RK_OK
    assert bool((dgl == 0).all()) and bool((dz == 1.0).all())  # equal experts: no gate gradient; sum_k g dm = 1

    w = [torch.ones(Hh, device=DEV) for _ in range(K)]
    dl, pr = torch.ones(B, K, device=DEV), torch.full((B, K), 0.5, device=DEV)
    gout, dt = torch.full((B, 4), SENTINEL, device=DEV), torch.full((B, K * Hh), SENTINEL, device=DEV)

    def head(K=K, dl_=dl.data_ptr(), dt_=dt.data_ptr()):
        return lib.rk_mmoe_head_backward(B, K, Hh, Hh, dl_, None, pr.data_ptr(), _ptrs((w * 5)[:K]),
                                         None, 1.0, gout.data_ptr(), 4 if K <= 4 else 12, dt_, 0, st)
    assert head(dl_=None) == INVALID and "rk_mmoe_head_backward" in _lib.last_error()
    assert head(K=9) == _lib.RK_ERR_UNSUPPORTED
    assert head(dt_=dt.data_ptr() + 2) == INVALID
    torch.cuda.synchronize()
    assert bool((gout == SENTINEL).all()) and bool((dt == SENTINEL).all())
    assert head() == _lib.RK_OK
    assert bool((dt == 1.0).all()) and bool((gout[:, :K] == 1.0).all()) and bool((gout[:, K:] == 0).all())


def test_train_forward_envelope():
    lib = _lib.load()
    dev = torch.device(DEV)
    _lib.ensure_device(dev)
    width, E, K, n = 20, 2, 2, 16
    x = torch.ones(4, width, device=DEV)
    img = [torch.zeros(64, 64, device=DEV) for _ in range(E)]
    stacks = [[(img[e], None, n, "relu")] for e in range(E)]
    gate = torch.zeros(64, 64, device=DEV)
    sh = ops.MmoeShape(width, E, K, (n,), (), False)
    args, keep = ops.mmoe_forward_args([ops.dense_segment(x, width, 0)], width, 4, stacks, gate, None, K, None, None, dev)
    xo, ea = torch.full((4, width), SENTINEL, device=DEV), torch.full((4, E * n), SENTINEL, device=DEV)
    mixed, gp = torch.full((4, K * n), SENTINEL, device=DEV), torch.full((4, K, E), SENTINEL, device=DEV)

    def call(p=0.0, xo_=xo.data_ptr(), ea_=ea.data_ptr()):
        return lib.rk_mmoe_forward_train(*args[:14], p, 0, None, xo_, _ptrs([ea_]), None, None, None, mixed.data_ptr(),
                                         gp.data_ptr(), _lib.raw_stream(dev))
    assert call(xo_=None) == INVALID and "rk_mmoe_forward_train" in _lib.last_error()
    assert call(p=0.5) == INVALID          # dropout without a stream slot
    assert call(ea_=ea.data_ptr() + 4) == INVALID
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (xo, ea, mixed, gp))
    assert call() == _lib.RK_OK
    assert bool((xo == 1).all()) and bool((ea == 0).all()) and bool((gp == 0.5).all()) and bool((mixed == 0).all())
    assert sh.zw == E * n + 4


# ---------------------------------------------------------------- the model

def engine_keeps(model, B):
    """The dropout multipliers the last train forward drew, by the documented site numbering."""
    slot = model._dropout.counter - 1
    sites = T.sites_of(model.num_experts, len(model.task_names), model.expert_hidden_units, model.tower_hidden_units)
    return {s: ops.dropout_mask(model._dropout.seed + s, slot, B, n, model.dropout_rate).cpu().double() for s, n in sites}


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
        if a.grad is None:
            continue
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
    torch.nn.BCEWithLogitsLoss(reduction="sum")(logits, torch.zeros(0, K, device=DEV)).backward()
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
    assert not torch.equal(fresh.experts[0][0].weight, a.experts[0][0].weight.cpu())
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
