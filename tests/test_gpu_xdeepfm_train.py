"""GPU tests of xDeepFM training: rk_cin_forward_train / rk_cin_backward / rk_cin_wgrad at op level
(through rankops.cin under autograd) and rankops.XDeepFM(trainable=True) at model level, against the
float64 restatement in tests/xdeepfm_train_ref.py with the gradient tolerance derived there (50 x the
restatement's own float32 drift, relative to each tensor's largest reference value).

Which op-level case reaches which path of rk_cin_backward (its tile is chosen as the forward's):
  wechat_b1, wechat_b7   batch * D <= 64: the 64-column tile, a partial sample tile
  wechat_b33, off_grid   128-column tile with padded rows, two / one workgroups; off_grid: H 5 / 17 / 1
                         (row tiles with 11 / 15 / 15 dead rows, K loops of one and two 16-blocks), D 4
  most_fields            four layers, m 32 (eight field groups of four), 128-column tile
  wide_k                 LDS forces the 64-column tile with padded rows; a sample spans two 16-column tiles
  widest                 H 256 with m 2 (a two-field tail group): the 64-column tile with unpadded rows
rk_cin_wgrad: 64 reduction columns per step, at most 32 slabs.  Every OP_CASES batch is one slab per
tile; T.SLAB_CASE (B 1,000 at the wechat shape: 125 tiles of 8 samples, 4 tiles per slab) spans 32 slabs
whose last one holds a single tile.  wide_k covers 30 column blocks of 128 (the last one partial),
widest 16 row tiles, off_grid rows and columns off the 16 grid."""
import functools

import pytest
import torch

import helpers as H
import rankops
import xdeepfm_ref as X
import xdeepfm_train_ref as T
from rankops import _lib, ops
from test_gpu_train import _assert_adam_params_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_IDS = [c[0] for c in X.OP_CASES]


def on_gpu(obj):
    return [on_gpu(o) for o in obj] if isinstance(obj, (list, tuple)) else obj.to(DEV)


@functools.lru_cache(maxsize=None)
def plain_reference(case, act):
    return T.op_grads(case, act, torch.float64)


def run_op(case, act, output_layer=True, conv=False, strided_grad=False):
    """rankops.cin under autograd on the case's seeded inputs (rows with stride m D + ROW_PAD) and
    the op-level loss; returns the same dict as T.op_grads, on the CPU."""
    _, m, D, _, B = case
    rows, Ws, bs, out_w, out_b = on_gpu(X.op_inputs(case))
    G, g = on_gpu(T.loss_weights(case))
    rows.requires_grad_(True)
    if conv:
        Ws = [w.unsqueeze(2) for w in Ws]
    for t in (*Ws, *bs, out_w, out_b):
        t.requires_grad_(True)
    assert rows.stride(0) == m * D + X.ROW_PAD  # a row stride larger than m * D
    x0 = rows[:, :m * D].view(B, m, D)
    if output_layer:
        pooled, logit, maps = rankops.cin(x0, Ws, bs, act, out_w, out_b, return_maps=True)
    else:
        (pooled, maps), logit = rankops.cin(x0, Ws, bs, act, return_maps=True), None
    assert pooled.requires_grad and not any(t.requires_grad for t in maps)
    if strided_grad:  # a gradient of pooled with a column stride of 2
        wide = torch.zeros(B, 2 * G.shape[1], device=DEV)
        wide[:, ::2] = G
        grads = [wide[:, ::2]]
        assert not grads[0].is_contiguous()
    else:
        grads = [G]
    outs = [pooled]
    if output_layer:
        outs.append(logit)
        grads.append(g)
    torch.autograd.backward(outs, grads)
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.detach().cpu()  # noqa: E731
    return dict(pooled=cpu(pooled), logit=cpu(logit), maps=[cpu(t) for t in maps],
                dx0=rows.grad[:, :m * D].reshape(B, m, D).cpu(), pad_grad=rows.grad[:, m * D:].cpu(),
                dW=[cpu(w.grad) for w in Ws], dbias=[cpu(b.grad) for b in bs],
                dout_w=cpu(out_w.grad) if output_layer else None, dout_b=cpu(out_b.grad) if output_layer else None)


def reference_for(case, act, got, output_layer=True):
    """The float64 reference differentiated with the engine's ReLU pattern (maps > 0), after checking
    that pattern against the reference's own sign outside the near-kink band and the maps themselves."""
    plain = plain_reference(case, act)
    for k, (mk, rk, yk) in enumerate(zip(got["maps"], plain["maps"], plain["pre"])):
        assert mk.shape == rk.shape
        torch.testing.assert_close(mk.double(), rk, atol=X.POOLED_TOL, rtol=X.POOLED_TOL, msg=lambda s: f"maps {k}: {s}")
        if act == "relu":
            band = T.near_kink(yk)
            assert bool(((mk > 0) == (yk > 0))[~band].all()), f"layer {k}: ReLU pattern differs outside the band"
    if act != "relu":
        return plain if output_layer else T.op_grads(case, act, torch.float64, output_layer=False)
    masks = [mk > 0 for mk in got["maps"]]
    if output_layer and all(torch.equal(a, y > 0) for a, y in zip(masks, plain["pre"])):
        return plain
    return T.op_grads(case, act, torch.float64, masks=masks, output_layer=output_layer)


def check_grads(got, want, what):
    for (name, g), (_, w) in zip(T.grad_tensors(got), T.grad_tensors(want)):
        g = g.reshape(w.shape)
        top = float(w.abs().max())
        if top == 0.0:
            assert not bool(g.any()), f"{what} {name}: the reference is all zero"
            continue
        err = T.grad_err(g, w)
        print(f"{what} {name}: err {err:.3g} (tol {T.GRAD_TOL:.3g})")
        assert err <= T.GRAD_TOL, f"{what} {name}: max |err| / max |want| = {err:.3g} > {T.GRAD_TOL:.3g}"


# ---------------------------------------------------------------- op level

@pytest.mark.parametrize("act", X.ACTIVATIONS)
@pytest.mark.parametrize("case", X.OP_CASES, ids=CASE_IDS)
def test_cin_gradients_match_float64(case, act):
    got = run_op(case, act)
    want = reference_for(case, act, got)
    torch.testing.assert_close(got["pooled"].double(), want["pooled"], atol=X.POOLED_TOL, rtol=X.POOLED_TOL)
    torch.testing.assert_close(got["logit"].double(), want["logit"], atol=X.LOGIT_TOL, rtol=X.LOGIT_TOL)
    check_grads(got, want, f"{case[0]} {act}")
    assert not bool(got["pad_grad"].any())  # the columns past m D of the row buffer are not x0
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("act", X.ACTIVATIONS)
def test_reduction_slabs(act):
    """B 1,000 at the wechat shape: 125 reduction tiles of 8 samples -> 4 tiles per slab, 32 slabs,
    the last with one tile (rk_cin_wgrad: 64 columns per tile, at most 32 slabs)."""
    got = run_op(T.SLAB_CASE, act)
    check_grads(got, reference_for(T.SLAB_CASE, act, got), f"slabs {act}")


def test_bit_equality_and_input_forms():
    case = X.OP_CASES[2]  # wechat_b33
    _, m, D, _, B = case
    a, b = run_op(case, "relu"), run_op(case, "relu")
    for (name, x), (_, y) in zip(T.grad_tensors(a), T.grad_tensors(b)):
        assert torch.equal(x, y), f"{name}: two backward calls differ"
    rows, Ws, bs, out_w, out_b = on_gpu(X.op_inputs(case))
    with torch.no_grad():
        pooled, logit = rankops.cin(rows[:, :m * D].view(B, m, D), Ws, bs, "relu", out_w, out_b)
    assert torch.equal(pooled.cpu(), a["pooled"]) and torch.equal(logit.cpu(), a["logit"])
    # a non-contiguous gradient of pooled, Conv1d-shaped weights
    c = run_op(case, "relu", conv=True, strided_grad=True)
    assert [tuple(t.shape) for t in c["dW"]] == [(128, 36, 1), (128, 768, 1)]
    for (name, x), (_, y) in zip(T.grad_tensors(a), T.grad_tensors(c)):
        assert torch.equal(x, y.reshape(x.shape)), f"{name}: input form changed the bits"
    # pooled alone, no output layer
    for cs in (case, X.OP_CASES[3]):
        d = run_op(cs, "relu", output_layer=False)
        assert d["logit"] is None and d["dout_w"] is None
        check_grads(d, reference_for(cs, "relu", d, output_layer=False), f"{cs[0]} pooled only")
    # return_maps on the plain path: the same maps, no graph
    with torch.no_grad():
        _, _, maps = rankops.cin(rows[:, :m * D].view(B, m, D), Ws, bs, "relu", out_w, out_b, return_maps=True)
    assert all(torch.equal(x.cpu(), y) for x, y in zip(maps, a["maps"]))
    assert rankops.error_flags() == 0


def test_tile_paths_agree():
    """off_grid (B 37, D 4: the 128-column tile) and its first 16 samples alone (batch * D = 64: the
    64-column tile) are both within GRAD_TOL of one float64 value per element of dx0."""
    case = X.OP_CASES[3]
    _, m, D, _, B = case
    rows, Ws, bs, out_w, out_b = on_gpu(X.op_inputs(case))
    G, g = on_gpu(T.loss_weights(case))
    dx = []
    for n in (B, 16):
        x0 = rows[:n, :m * D].reshape(n, m, D).clone().requires_grad_(True)
        pooled, logit = rankops.cin(x0, Ws, bs, "relu", out_w, out_b)
        torch.autograd.backward([pooled, logit], [G[:n], g[:n]])
        dx.append(x0.grad.cpu())
    want = plain_reference(case, "relu")["dx0"]
    assert float((dx[0][:16] - dx[1]).abs().max()) <= 2 * T.GRAD_TOL * float(want.abs().max())


def raw_backward(m=6, D=8, maps=(16,), B=4, batch=None, null=None, misalign=None):
    """rk_cin_backward's and rk_cin_wgrad's status over valid zero buffers of the given shape."""
    lib = _lib.load()
    dev = torch.device(DEV)
    _lib.ensure_device(dev)
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    hs = sum(maps)
    x0, dx0, saved, dy, dpooled = z(B, m * D), torch.full((B, m * D), 7.0, device=DEV), z(B, hs, D), z(B, hs, D), z(B, hs)
    hprev, images = m, []
    for h in maps:
        images.append(z(m * ((hprev + 15) // 16 * 16) * ((h + 15) // 16 * 16) + 4))
        hprev = h
    nl = len(maps)
    wp = (ops.ctypes.c_void_p * nl)(*[t.data_ptr() + (4 if misalign == "image" else 0) for t in images])
    sz = (ops.ctypes.c_int32 * nl)(*maps)
    n = B if batch is None else batch
    rc_b = lib.rk_cin_backward(None if null == "x0" else x0.data_ptr() + (4 if misalign == "x0" else 0), m * D, m, D, n,
                               None if null == "images" else wp, sz, nl, _lib.RK_ACT_RELU, saved.data_ptr(),
                               None if null == "grad" else dpooled.data_ptr(), hs, None, None, None, 0,
                               None if null == "dx0" else dx0.data_ptr(), m * D, dy.data_ptr(), _lib.raw_stream(dev))
    err_b = _lib.last_error()
    hprev, dws, dbs = m, [], []
    for h in maps:
        dws.append(torch.full((h, hprev * m), 7.0, device=DEV))
        dbs.append(torch.full((h,), 7.0, device=DEV))
        hprev = h
    ws = ops.cin_wgrad_workspace(m, maps, dev) if 1 <= nl <= 4 and m > 0 else z(4)
    dwp = (ops.ctypes.c_void_p * nl)(*[t.data_ptr() for t in dws])
    dbp = (ops.ctypes.c_void_p * nl)(*[t.data_ptr() for t in dbs])
    rc_w = lib.rk_cin_wgrad(None if null == "x0" else x0.data_ptr() + (4 if misalign == "x0" else 0), m * D, m, D, n,
                            sz, nl, saved.data_ptr(), dy.data_ptr(), None if null == "dw" else dwp, dbp, ws.data_ptr(),
                            ws.numel(), _lib.raw_stream(dev))
    torch.cuda.synchronize()
    return rc_b, rc_w, dx0, dws, dbs, err_b


def test_status_codes():
    OK, INVALID, UNSUPPORTED = _lib.RK_OK, 1, _lib.RK_ERR_UNSUPPORTED
    rc_b, rc_w, dx0, dws, dbs, _ = raw_backward()
    assert (rc_b, rc_w) == (OK, OK)
    assert not bool(dx0.any()) and not bool(dws[0].any()) and not bool(dbs[0].any())  # zero gradients in, zero out
    assert raw_backward(D=12)[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert raw_backward(maps=(16,) * 5)[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert raw_backward(maps=(257,))[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert raw_backward(m=33)[:2] == (UNSUPPORTED, UNSUPPORTED)
    assert raw_backward(m=1)[:2] == (UNSUPPORTED, UNSUPPORTED)
    for what in ("x0", "images", "grad", "dx0"):
        rc_b, _, dx0, _, _, err = raw_backward(null=what)
        assert rc_b == INVALID and "rk_cin_backward" in err, what
        assert bool((dx0 == 7.0).all())  # nothing was launched
    assert raw_backward(null="x0")[1] == INVALID and raw_backward(null="dw")[1] == INVALID
    assert raw_backward(misalign="image")[0] == INVALID
    assert raw_backward(misalign="x0")[:2] == (INVALID, INVALID)
    assert raw_backward(batch=-1)[:2] == (INVALID, INVALID)
    rc_b, rc_w, dx0, dws, dbs, _ = raw_backward(batch=0)
    assert (rc_b, rc_w) == (OK, OK) and bool((dx0 == 7.0).all())
    assert not bool(dws[0].any()) and not bool(dbs[0].any())  # an empty batch: zeroed weight gradients
    # the packer and the train forward
    lib = _lib.load()
    w, out = torch.zeros(16, 36, device=DEV), torch.zeros(6 * 16 * 16 + 4, device=DEV)
    st = _lib.raw_stream(torch.device(DEV))
    assert lib.rk_cin_pack_weight_t(w.data_ptr(), 36, 16, 6, 6, out.data_ptr(), st) == OK
    assert lib.rk_cin_pack_weight_t(None, 36, 16, 6, 6, out.data_ptr(), st) == INVALID
    assert lib.rk_cin_pack_weight_t(w.data_ptr(), 36, 16, 6, 6, out.data_ptr() + 4, st) == INVALID
    assert lib.rk_cin_pack_weight_t(w.data_ptr(), 35, 16, 6, 6, out.data_ptr(), st) == INVALID
    x = torch.zeros(4, 48, device=DEV)
    segs = [ops.dense_segment(x, 8, i * 8, i * 8) for i in range(6)]
    args, _keep = ops.cin_forward_args(segs, None, 8, 4, [torch.zeros(16 * 48, device=DEV)], [None], (16,), "identity",
                                       None, None, None, None, None, None, torch.device(DEV))
    args[-1:] = [None, st]
    assert lib.rk_cin_forward_train(*args) == INVALID  # no maps buffer
    empty = rankops.cin(torch.zeros(0, 6, 8, device=DEV, requires_grad=True),
                        [torch.zeros(16, 36, device=DEV, requires_grad=True)], None)
    empty.sum().backward()
    assert empty.shape == (0, 16)
    assert rankops.error_flags() == 0


# ---------------------------------------------------------------- model level

WECHAT = {f: H.WECHAT_VOCAB[f] for f in rankops.deepfm.WECHAT_FIELDS}
STEP_CONFIGS = {
    "wechat_identity": dict(sizes=WECHAT, D=8, act="identity", bn=True, B=256),
    "wechat_relu": dict(sizes=WECHAT, D=8, act="relu", bn=True, B=256),
    "no_batch_norm": dict(sizes=WECHAT, D=8, act="relu", bn=False, B=256),
    "wide_b64": dict(sizes=X.WIDE_FIELDS, D=32, act="relu", bn=True, B=64),
}


def build(cfg, seed=42, **kw):
    torch.manual_seed(seed)
    model = rankops.XDeepFM(None, embedding_dim=cfg["D"], cin_activation=cfg["act"], batch_norm=cfg["bn"],
                            vocab_sizes=cfg["sizes"], **kw)
    return H.randomize_eval_stats(model, seed + 1)


def dropout_masks(model, B):
    """The dropout multipliers the last train forward drew (as tests/test_gpu_train.py's _deepfm_masks)."""
    from rankops import train as rt
    slot = model._dropout.counter - 1
    return [ops.dropout_mask(model._dropout.seed + u, slot, B, lin.out_features, p).cpu() if p > 0 else None
            for u, (lin, bn, relu, p) in enumerate(rt.deep_units(model.deep_layers))]


def relu_masks(model, dcat):
    """The CIN's ReLU pattern of this step: rankops.cin on the torch-gathered rows with the current
    weights (the forward is deterministic: the model's own maps have these bits)."""
    with torch.no_grad():
        x0 = torch.stack([model.second_order_embeddings[n].weight[dcat[n]] for n in model.second_order_embeddings], 1)
        *_, maps = rankops.cin(x0, [c.weight for c in model.cin_layers], [c.bias for c in model.cin_layers],
                               model.cin_activation, return_maps=True)
    return [(t > 0).cpu() for t in maps]


@pytest.mark.parametrize("name", list(STEP_CONFIGS))
def test_xdeepfm_train_steps_match_autograd(name):
    cfg = STEP_CONFIGS[name]
    B, steps = cfg["B"], 3
    model = build(cfg, trainable=True).to(DEV).train()
    cat = H.deepfm_inputs(B, cfg["sizes"], 2300)["category"]
    dcat = H.to_device(cat, DEV)
    label = (torch.rand(B, generator=torch.Generator().manual_seed(2300)) < 0.3).double()
    params = dict(model.named_parameters())
    p = {k: (v.detach().cpu().double().requires_grad_(True) if k in params else
             (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu().clone()))
         for k, v in model.state_dict().items()}
    names = list(params)
    opt = rankops.Adam(model.parameters(), lr=1e-3)
    ref_opt = torch.optim.Adam([p[n] for n in names], lr=1e-3)
    crit = torch.nn.BCELoss()
    layers = list(model.deep_layers)
    bn_fed_biases = {f"deep_layers.{i}.bias" for i, m in enumerate(layers[:-1])
                     if isinstance(m, torch.nn.Linear) and isinstance(layers[i + 1], torch.nn.BatchNorm1d)}
    for step in range(steps):
        opt.zero_grad()
        ref_opt.zero_grad()
        cin_masks = relu_masks(model, dcat) if cfg["act"] == "relu" else None
        out = model(dcat)
        assert len(out) == 5 and all(o.shape == (B, 1) and o.requires_grad for o in out)
        crit(out[0].squeeze(), label.float().to(DEV)).backward()
        ref = T.forward_train(p, cat, cfg["act"], cin_masks, 3, cfg["bn"], 0.1, dropout_masks(model, B))
        crit(ref[0].squeeze(), label).backward()
        for i, (o, r) in enumerate(zip(out, ref)):
            torch.testing.assert_close(o.detach().cpu().double(), r.detach(), rtol=1e-4, atol=1e-4, msg=f"output {i}")
        for k, v in model.state_dict().items():
            if k not in params and (step == 0 or not k.endswith("running_mean")):
                torch.testing.assert_close(v.cpu().to(p[k].dtype), p[k], rtol=1e-4, atol=1e-5, msg=f"buffer {k} step {step}")
        for n, prm in model.named_parameters():
            want = p[n].grad
            scale = max(1e-3, float(want.abs().max()))
            torch.testing.assert_close(prm.grad.cpu().double(), want, rtol=0, atol=5e-4 * scale,
                                       msg=lambda s: f"grad {n} step {step}: {s}")
        opt.step()
        ref_opt.step()
        for n, prm in model.named_parameters():
            if n in bn_fed_biases:  # zero true gradient: rounding noise that Adam turns into +-lr steps
                continue
            _assert_adam_params_close(prm.detach().cpu().double(), p[n].detach(), lr=1e-3, steps=1,
                                      what=f"param {n} after step {step}")
        with torch.no_grad():  # re-synchronise the reference to the engine (see _deepfm_step_check)
            for k, v in model.state_dict().items():
                p[k].copy_(v.cpu())
            for n, prm in model.named_parameters():
                for key in ("exp_avg", "exp_avg_sq"):
                    ref_opt.state[p[n]][key].copy_(opt.state[prm][key].cpu())
    assert rankops.error_flags() == 0


def is_table(model, prm):
    return any(prm is e.weight for d in (model.first_order_embeddings, model.second_order_embeddings) for e in d.values())


def test_sparse_gradients_equal_the_dense_ones():
    cfg = STEP_CONFIGS["wechat_relu"]
    dense = build(cfg, trainable=True).to(DEV).train()
    sparse = build(cfg, trainable=True, sparse_grad=True).to(DEV).train()
    sparse.load_state_dict(dense.state_dict())
    B = 64
    dcat = H.to_device(H.deepfm_inputs(B, cfg["sizes"], 11)["category"], DEV)
    label = (torch.rand(B, generator=torch.Generator().manual_seed(3)) < 0.3).float().to(DEV)
    for model in (dense, sparse):
        torch.manual_seed(5)  # the dropout streams' seed
        torch.nn.BCELoss()(model(dcat)[0].squeeze(), label).backward()
    tables = 0
    for (n, a), b in zip(dense.named_parameters(), sparse.parameters()):
        scale = max(1e-3, float(a.grad.abs().max()))
        g = b.grad
        if is_table(dense, a):
            tables += 1
            assert g.is_sparse and g.shape == a.shape and g._nnz() == B, n
            g = g.to_dense()
        torch.testing.assert_close(g, a.grad, rtol=0, atol=2e-4 * scale, msg=lambda s: f"{n}: {s}")
    assert tables == 12
    tabs = [q for q in sparse.parameters() if is_table(sparse, q)]
    before = [q.detach().clone() for q in tabs]
    rankops.SparseAdam(tabs, lr=1e-3).step()
    assert all(not torch.equal(x, q.detach()) for x, q in zip(before, tabs))
    assert rankops.error_flags() == 0


def test_graph_capture_replays_follow_the_weights():
    """One captured train step replayed with fresh inputs against an eager twin: a weight image
    packed on the host, outside the graph, would go stale after the first Adam step."""
    cfg = dict(STEP_CONFIGS["wechat_relu"], B=64)
    B = cfg["B"]
    a, b = build(cfg, trainable=True).to(DEV).train(), build(cfg, trainable=True).to(DEV).train()
    oa = rankops.Adam(a.parameters(), lr=1e-3, capturable=True)
    ob = rankops.Adam(b.parameters(), lr=1e-3, capturable=True)
    batches = [H.to_device(H.deepfm_inputs(B, cfg["sizes"], 50 + i)["category"], DEV) for i in range(6)]
    labels = [(torch.rand(B, generator=torch.Generator().manual_seed(50 + i)) < 0.3).float().to(DEV) for i in range(6)]
    layers = list(a.deep_layers)
    bn_fed_biases = {f"deep_layers.{i}.bias" for i, m in enumerate(layers[:-1])
                     if isinstance(m, torch.nn.Linear) and isinstance(layers[i + 1], torch.nn.BatchNorm1d)}
    static = {k: v.clone() for k, v in batches[0].items()}
    static_label = labels[0].clone()
    crit = torch.nn.BCELoss()

    def step(model, opt, cat, label):
        opt.zero_grad(set_to_none=True)
        loss = crit(model(cat)[0].squeeze(), label)
        loss.backward()
        opt.step()
        return loss

    def feed(i):
        for k in static:
            static[k].copy_(batches[i][k])
        static_label.copy_(labels[i])

    torch.manual_seed(9)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(2):
            feed(i)
            step(a, oa, static, static_label)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    oa.zero_grad(set_to_none=True)
    feed(2)
    with torch.cuda.graph(graph):
        step(a, oa, static, static_label)
    torch.manual_seed(9)
    for i in range(2):
        step(b, ob, batches[i], labels[i])
    for i in range(2, 6):  # four replays, each on its own batch
        feed(i)
        graph.replay()
        step(b, ob, batches[i], labels[i])
        torch.cuda.synchronize()
        for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
            if n in bn_fed_biases:  # zero true gradient: rounding noise that Adam turns into +-lr steps
                continue
            _assert_adam_params_close(pa.detach().cpu(), pb.detach().cpu(), lr=1e-3, steps=i + 1,
                                      what=f"{n} after replay {i - 1}")
    # the CIN weights moved, and the replays saw them move
    fresh = build(cfg, trainable=True)
    assert not torch.equal(fresh.cin_layers[0].weight, a.cin_layers[0].weight.cpu())
    assert rankops.error_flags() == 0


def test_eval_after_training_and_no_grad_train_mode():
    cfg = STEP_CONFIGS["wechat_relu"]
    B = 128
    model = build(cfg, trainable=True).to(DEV).train()
    cat = H.deepfm_inputs(B, cfg["sizes"], 77)["category"]
    dcat = H.to_device(cat, DEV)
    label = (torch.rand(B, generator=torch.Generator().manual_seed(77)) < 0.3).float().to(DEV)
    with torch.no_grad():
        model.eval()(dcat)  # an eval forward first: its cached weight images must not outlive the steps
    model.train()
    opt = rankops.Adam(model.parameters(), lr=1e-2)
    for _ in range(3):
        opt.zero_grad()
        torch.nn.BCELoss()(model(dcat)[0].squeeze(), label).backward()
        opt.step()
    with torch.no_grad():  # train mode without autograd: outputs only, nothing kept
        out = model(dcat)
    assert len(out) == 5 and all(o.shape == (B, 1) and not o.requires_grad and o.grad_fn is None for o in out)
    assert all(bool(torch.isfinite(o).all()) for o in out)
    model.eval()
    ref = X.forward(X.floats(H.cpu_params(model), torch.float64), cat, "relu")
    with torch.no_grad():
        got = model(dcat)
        prepared = model.prepare(dcat)()
    names = ("probability", "total_logit", "linear_logit", "cin_logit", "deep_logit")
    for name, o, q, r in zip(names, got, prepared, ref):
        tol = X.PROB_TOL if name == "probability" else X.LOGIT_TOL
        torch.testing.assert_close(o.cpu().double(), r, atol=tol, rtol=tol, msg=lambda s: f"{name}: {s}")
        assert torch.equal(o, q), name
    assert rankops.error_flags() == 0


def test_training_stays_opt_in():
    cfg = STEP_CONFIGS["wechat_identity"]
    default, opted = build(cfg), build(cfg, trainable=True)
    assert not default.trainable and opted.trainable and not opted.sparse_grad
    assert list(default.state_dict()) == list(opted.state_dict())
    for (k, v), w in zip(default.state_dict().items(), opted.state_dict().values()):
        assert torch.equal(v, w), k
    dcat = H.to_device(H.deepfm_inputs(8, cfg["sizes"], 1)["category"], DEV)
    default = default.to(DEV).train()
    with pytest.raises(NotImplementedError):
        default(dcat)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        default(dcat)
    torch.manual_seed(42)
    deepfm = rankops.DeepFM(None, vocab_sizes=cfg["sizes"])
    res = opted.load_state_dict(deepfm.state_dict(), strict=False)
    assert not res.unexpected_keys and all(k.startswith(("cin_layers.", "cin_output_layer.")) for k in res.missing_keys)
    empty = opted.to(DEV).train()({k: v[:0] for k, v in dcat.items()})
    assert len(empty) == 5 and all(o.shape == (0, 1) for o in empty)
