"""GPU tests of xDeepFM: rk_cin_forward at op level (dense segments, through rankops.cin) and
rankops.XDeepFM at model level, against the float64 restatement in tests/xdeepfm_ref.py with the
tolerances derived there (50 x the restatement's own float32 drift)."""
import functools

import pytest
import torch

import helpers as H
import rankops
import xdeepfm_ref as X
from rankops import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_IDS = [c[0] for c in X.OP_CASES]
WECHAT_300 = X.MODEL_CASES[1]


@functools.lru_cache(maxsize=None)
def op_reference(case, act):
    return X.op_reference(case, act)


def close(got, ref, tol, what):
    got = got.detach().cpu()
    print(f"{what}: err {X.rel_err(got, ref):.3g} (tol {tol:.3g})")
    torch.testing.assert_close(got.double(), ref, atol=tol, rtol=tol, msg=lambda m: f"{what}: {m}")


def on_gpu(obj):
    return [on_gpu(o) for o in obj] if isinstance(obj, (list, tuple)) else obj.to(DEV)


def run_op(case, act):
    _, m, D, _, B = case
    rows, Ws, bs, out_w, out_b = on_gpu(X.op_inputs(case))
    assert rows.stride(0) == m * D + X.ROW_PAD  # a row stride larger than m * D
    x0 = rows[:, :m * D].view(B, m, D)
    return rankops.cin(x0, Ws, bs, act, out_w, out_b)


@pytest.mark.parametrize("act", X.ACTIVATIONS)
@pytest.mark.parametrize("case", X.OP_CASES, ids=CASE_IDS)
def test_cin_matches_restatement(case, act):
    pooled, logit = run_op(case, act)
    ref_pooled, ref_logit = op_reference(case, act)
    assert pooled.shape == ref_pooled.shape and logit.shape == (case[4], 1)
    close(pooled, ref_pooled, X.POOLED_TOL, "pooled")
    close(logit, ref_logit, X.LOGIT_TOL, "cin_logit")
    again_pooled, again_logit = run_op(case, act)
    assert torch.equal(pooled, again_pooled) and torch.equal(logit, again_logit)  # fixed reduction order
    assert rankops.error_flags() == 0


def test_cin_without_output_layer_and_conv1d_weights():
    case = X.OP_CASES[3]
    _, m, D, _, B = case
    rows, Ws, bs, _, _ = on_gpu(X.op_inputs(case))
    pooled = rankops.cin(rows[:, :m * D].view(B, m, D), [w.unsqueeze(2) for w in Ws], bs, "relu")
    close(pooled, op_reference(case, "relu")[0], X.POOLED_TOL, "pooled")
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rankops.cin(rows.cpu()[:, :m * D].view(B, m, D), Ws, bs)


def raw_call(m=6, D=8, maps=(16,), B=4, null_segments=False, batch=None):
    """rk_cin_forward's status over valid dense buffers of the given shape."""
    lib = _lib.load()
    _lib.ensure_device(torch.device(DEV))
    x = torch.zeros(B, m * D, device=DEV)
    segs = [ops.dense_segment(x, D, i * D, i * D) for i in range(m)]
    hprev, images, biases = m, [], []
    for h in maps:
        images.append(torch.zeros((h + 15) // 16 * 16 * ((hprev * m + 15) // 16 * 16), device=DEV))
        biases.append(torch.zeros(h, device=DEV))
        hprev = h
    pooled = torch.full((B, sum(maps)), 7.0, device=DEV)
    args, _keep = ops.cin_forward_args(segs, None, D, B if batch is None else batch, images, biases, maps, "identity",
                                       None, None, None, None, pooled, None, torch.device(DEV))
    if null_segments:
        args[0] = None
    args[-1] = _lib.raw_stream(torch.device(DEV))
    rc = lib.rk_cin_forward(*args)
    torch.cuda.synchronize()
    return rc, pooled


def test_envelope_and_argument_errors():
    assert raw_call()[0] == _lib.RK_OK
    assert raw_call(m=33)[0] == _lib.RK_ERR_UNSUPPORTED
    assert raw_call(D=12)[0] == _lib.RK_ERR_UNSUPPORTED
    assert raw_call(maps=(16,) * 5)[0] == _lib.RK_ERR_UNSUPPORTED
    assert raw_call(maps=(257,))[0] == _lib.RK_ERR_UNSUPPORTED
    assert raw_call(m=1)[0] == _lib.RK_ERR_UNSUPPORTED
    rc, pooled = raw_call(null_segments=True)
    assert rc == 1 and "null" in _lib.last_error()
    assert bool((pooled == 7.0).all())  # nothing was launched
    rc, pooled = raw_call(batch=0)
    assert rc == _lib.RK_OK and bool((pooled == 7.0).all())
    assert raw_call(batch=-1)[0] == 1
    empty = rankops.cin(torch.zeros(0, 6, 8, device=DEV), [torch.zeros(16, 36, device=DEV)], None)
    assert empty.shape == (0, 16)
    assert rankops.error_flags() == 0


# ---------------------------------------------------------------- model level

@functools.lru_cache(maxsize=None)
def gpu_model(fields_key):
    case = next(c for c in X.MODEL_CASES if (c[1] is None) == (fields_key is None))
    model = X.build_model(case)
    params = X.floats(H.cpu_params(model), torch.float64)
    return model.to(DEV), params


def model_for(case):
    return gpu_model(None if case[1] is None else "wide")


@pytest.mark.parametrize("case", X.MODEL_CASES, ids=[c[0] for c in X.MODEL_CASES])
def test_model_matches_restatement(case):
    model, params = model_for(case)
    cat = X.model_inputs(case)
    ref = X.forward(params, cat)
    with torch.no_grad():
        out = model(H.to_device(cat, DEV))
    assert len(out) == 5
    names = ("probability", "total_logit", "linear_logit", "cin_logit", "deep_logit")
    for name, o, r in zip(names, out, ref):
        assert o.shape == (case[3], 1) and o.dtype == torch.float32
        close(o, r, X.PROB_TOL if name == "probability" else X.LOGIT_TOL, name)
    assert rankops.error_flags() == 0


def test_model_relu_activation():
    model = X.build_model(WECHAT_300, cin_activation="relu")
    params = X.floats(H.cpu_params(model), torch.float64)
    cat = X.model_inputs(WECHAT_300)
    ref = X.forward(params, cat, "relu")
    with torch.no_grad():
        out = model.to(DEV)(H.to_device(cat, DEV))
    close(out[3], ref[3], X.LOGIT_TOL, "cin_logit")
    close(out[1], ref[1], X.LOGIT_TOL, "total_logit")
    assert not torch.allclose(ref[3], X.forward(params, cat)[3])


def test_out_of_range_id_raises_the_flag():
    model, _ = model_for(WECHAT_300)
    cat = H.to_device(X.model_inputs(WECHAT_300), DEV)
    assert rankops.error_flags() == 0
    cat["feedid"][5] = model.vocab_sizes["feedid"]  # one past the last row
    with torch.no_grad():
        out = model(cat)
    assert rankops.error_flags() == _lib.RK_FLAG_INDEX_OOB
    assert all(bool(torch.isfinite(o).all()) for o in out)
    assert rankops.error_flags() == 0


def test_prepare_is_bit_equal_and_follows_its_inputs():
    model, _ = model_for(WECHAT_300)
    cat = H.to_device(X.model_inputs(WECHAT_300), DEV)
    with torch.no_grad():
        want = [o.clone() for o in model(cat)]
    run = model.prepare(cat)
    out = run()
    assert all(torch.equal(a, b) for a, b in zip(out, want))
    other = H.to_device(X.model_inputs(WECHAT_300, seed=77), DEV)
    for k in cat:
        cat[k].copy_(other[k])
    again = run()
    assert all(a is b for a, b in zip(again, out))  # the same output tensors on every run()
    with torch.no_grad():
        fresh = model(other)
    assert all(torch.equal(a, b) for a, b in zip(again, fresh))
    assert not torch.equal(fresh[0], want[0])
    assert rankops.error_flags() == 0


def test_forward_follows_an_in_place_weight_update():
    model = X.build_model(WECHAT_300).to(DEV)
    cat = X.model_inputs(WECHAT_300)
    dcat = H.to_device(cat, DEV)
    with torch.no_grad():
        before = [o.clone() for o in model(dcat)]
        model.cin_layers[0].weight.mul_(0.5)
        model.cin_layers[1].bias.add_(0.25)
        after = model(dcat)
    ref = X.forward(X.floats(H.cpu_params(model), torch.float64), cat)
    close(after[3], ref[3], X.LOGIT_TOL, "cin_logit after the update")
    close(after[1], ref[1], X.LOGIT_TOL, "total_logit after the update")
    assert not torch.equal(after[3], before[3])
    assert torch.equal(after[4], before[4])  # the deep part does not read the CIN weights


def test_deep_logit_is_bit_equal_to_deepfm():
    model, _ = model_for(WECHAT_300)
    torch.manual_seed(42)
    deepfm = rankops.DeepFM(None, vocab_sizes={f: H.WECHAT_VOCAB[f] for f in rankops.deepfm.WECHAT_FIELDS})
    deepfm = H.randomize_eval_stats(deepfm, 43).eval().to(DEV)
    cat = H.to_device(X.model_inputs(WECHAT_300), DEV)
    with torch.no_grad():
        ours, theirs = model(cat), deepfm(cat)
    assert torch.equal(ours[4], theirs[4])
    torch.testing.assert_close(ours[2], theirs[2], atol=X.LOGIT_TOL, rtol=X.LOGIT_TOL)  # the first-order sum


def test_train_mode_empty_batch_and_cpu_tensors():
    model = X.build_model(WECHAT_300).to(DEV)
    cat = X.model_inputs(WECHAT_300)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        model(cat)
    empty = model({k: v[:0] for k, v in H.to_device(cat, DEV).items()})
    assert len(empty) == 5 and all(o.shape == (0, 1) for o in empty)
    with pytest.raises(RuntimeError, match="eval mode"):
        model.train().prepare(H.to_device(cat, DEV))
    with pytest.raises(NotImplementedError):
        model(H.to_device(cat, DEV))
    with torch.no_grad(), pytest.raises(NotImplementedError):
        model(H.to_device(cat, DEV))
