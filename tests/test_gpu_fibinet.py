"""GPU tests of FiBiNET: rk_fibinet_interaction at op level (dense segments, through
rankops.fibinet_interaction) and rankops.FiBiNET at model level (the one-launch rk_fibinet_forward and the
two-launch path), against the float64 restatement in tests/fibinet_ref.py with the tolerances derived
there (50 x the restatement's own float32 drift, as rel_err = max |diff| / max |reference|)."""
import functools

import pytest
import torch

import fibinet_ref as X
import helpers as H
import rankops
from launch_count import launches_of
from rankops import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_IDS = [c[0] for c in X.OP_CASES]
MODEL_IDS = [c[0] for c in X.MODEL_CASES]
BY_NAME = {c[0]: c for c in X.MODEL_CASES}
WECHAT_300 = BY_NAME["wechat_b300_interaction"]
TWELVE = BY_NAME["twelve_b64"]
OUTPUTS = ("probability", "total_logit", "linear_logit", "deep_logit")


@functools.lru_cache(maxsize=None)
def op_reference(case, bilinear_type):
    return X.op_reference(case, bilinear_type)


def close(got, ref, tol, what):
    err = X.rel_err(got.detach().cpu(), ref)
    print(f"{what}: err {err:.3g} (tol {tol:.3g})")
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    assert err <= tol, (what, err, tol)


def on_gpu(obj):
    return [on_gpu(o) for o in obj] if isinstance(obj, (list, tuple)) else obj.to(DEV)


def run_op(case, bilinear_type):
    _, m, D, B = case
    rows, w1, w2, We, Wv = on_gpu(X.op_inputs(case, bilinear_type))
    assert rows.stride(0) == m * D + X.ROW_PAD  # a row stride larger than m * D
    x0 = rows[:, :m * D].view(B, m, D)
    return rankops.fibinet_interaction(x0, w1, w2, We, Wv, bilinear_type, return_attention=True)


@pytest.mark.parametrize("bilinear_type", X.BILINEAR_TYPES)
@pytest.mark.parametrize("case", X.OP_CASES, ids=CASE_IDS)
def test_interaction_matches_restatement(case, bilinear_type):
    c, a = run_op(case, bilinear_type)
    ref_c, ref_a = op_reference(case, bilinear_type)
    _, m, D, B = case
    assert c.shape == (B, m * (m - 1) * D) and a.shape == (B, m) and c.dtype == a.dtype == torch.float32
    close(c, ref_c, X.C_TOL, "c")
    close(a, ref_a, X.ATTN_TOL, "attention")
    again_c, again_a = run_op(case, bilinear_type)
    assert torch.equal(c, again_c) and torch.equal(a, again_a)  # fixed summation order
    assert rankops.error_flags() == 0


def test_interaction_without_attention_empty_batch_and_cpu_tensors():
    case = X.OP_CASES[1]
    _, m, D, B = case
    rows, w1, w2, We, Wv = on_gpu(X.op_inputs(case, "each"))
    x0 = rows[:, :m * D].view(B, m, D)
    c = rankops.fibinet_interaction(x0, w1, w2, We, Wv, "each")
    close(c, op_reference(case, "each")[0], X.C_TOL, "c")
    empty_c, empty_a = rankops.fibinet_interaction(x0[:0], w1, w2, We, Wv, "each", return_attention=True)
    assert empty_c.shape == (0, m * (m - 1) * D) and empty_a.shape == (0, m)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rankops.fibinet_interaction(x0.cpu(), w1, w2, We, Wv, "each")
    with pytest.raises(ValueError):
        rankops.fibinet_interaction(x0, w1, w2, We, Wv, "interaction")  # m - 1 matrices, not m (m - 1) / 2
    with pytest.raises(ValueError):
        rankops.fibinet_interaction(x0, w1, w2, We, Wv, "field")
    assert rankops.error_flags() == 0


def raw_call(m=6, D=8, r=2, B=4, null_segments=False, batch=None):
    """rk_fibinet_interaction's status over valid dense buffers of the given shape."""
    lib = _lib.load()
    _lib.ensure_device(torch.device(DEV))
    x = torch.zeros(B, m * D, device=DEV)
    segs = [ops.dense_segment(x, D, i * D, i * D) for i in range(m)]
    w1, w2 = torch.zeros(r, m, device=DEV), torch.zeros(m, r, device=DEV)
    be, bv = torch.zeros(1, D, D, device=DEV), torch.zeros(1, D, D, device=DEV)
    c = torch.full((B, max(1, m * (m - 1) * D)), 7.0, device=DEV)
    args, _keep = ops.fibinet_interaction_args(segs, None, D, B if batch is None else batch, w1, w2, be, bv, "all", c,
                                               None, None, torch.device(DEV))
    if null_segments:
        args[0] = None
    args[-1] = _lib.raw_stream(torch.device(DEV))
    rc = lib.rk_fibinet_interaction(*args)
    torch.cuda.synchronize()
    return rc, c


def test_envelope_and_argument_errors():
    rc, c = raw_call()
    assert rc == _lib.RK_OK and bool((c == 0.0).all())  # zero rows: a zero interaction vector
    for kw in (dict(m=33), dict(m=1), dict(D=6), dict(D=68), dict(r=33)):
        rc, c = raw_call(**kw)
        assert rc == _lib.RK_ERR_UNSUPPORTED, kw
        assert bool((c == 7.0).all())  # nothing was launched
    rc, c = raw_call(null_segments=True)
    assert rc == 1 and "null" in _lib.last_error()
    assert bool((c == 7.0).all())
    rc, c = raw_call(batch=0)
    assert rc == _lib.RK_OK and bool((c == 7.0).all())
    assert raw_call(batch=-1)[0] == 1
    assert rankops.error_flags() == 0


# ---------------------------------------------------------------- model level

@functools.lru_cache(maxsize=None)
def gpu_model(key):
    """One model per (fields, D, bilinear type, kwargs): the batch sizes of a shape share it."""
    case = next(c for c in X.MODEL_CASES if model_key(c) == key)
    model = X.build_model(case)
    params = X.floats(H.cpu_params(model), torch.float64)
    return model.to(DEV), params


def model_key(case):
    return (None if case[1] is None else tuple(case[1]), case[2], case[4], repr(case[5]))


def model_for(case):
    return gpu_model(model_key(case))


@functools.lru_cache(maxsize=None)
def model_reference(name):
    case = BY_NAME[name]
    return X.forward(model_for(case)[1], X.model_inputs(case))


def check_outputs(out, ref, B):
    assert len(out) == 4
    for name, o, r in zip(OUTPUTS, out, ref):
        assert o.shape == (B, 1) and o.dtype == torch.float32
        close(o, r, X.PROB_TOL if name == "probability" else X.LOGIT_TOL, name)


@pytest.mark.parametrize("case", X.MODEL_CASES, ids=MODEL_IDS)
def test_model_matches_restatement(case):
    model, _ = model_for(case)
    cat = H.to_device(X.model_inputs(case), DEV)
    with torch.no_grad():
        out = model(cat)
    check_outputs(out, model_reference(case[0]), case[3])
    assert model.fused() == (case[0] != "twelve_b64")
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("name", ["wechat_b300_all", "wechat_b300_each", "wechat_b300_interaction", "no_bn_b33",
                                  "d32_b64"])
def test_fused_forward_is_one_launch_and_agrees_with_two_launches(name):
    case = BY_NAME[name]
    model, _ = model_for(case)
    cat = H.to_device(X.model_inputs(case), DEV)
    with torch.no_grad():
        one = model(cat)  # (the first call builds and caches the launch: torch.cat of the bilinear matrices)
        names = launches_of(lambda: model(cat))
        print(names)
        assert names == ["rk_fibinet_forward"]
        model.two_launch = True
        try:
            two = model(cat)
            names = launches_of(lambda: model(cat))
        finally:
            model.two_launch = None
        print(names)
    assert names[0] == "rk_fibinet_interaction" and len(names) > 1 and "rk_fibinet_forward" not in names
    check_outputs(two, model_reference(name), case[3])
    for what, a, b in zip(OUTPUTS, one, two):
        close(a, b.cpu().double(), X.PROB_TOL if what == "probability" else X.LOGIT_TOL, f"{what}: one launch vs two")
    assert torch.equal(one[2], two[2])  # linear_logit: the same sum in the same order
    # deep_logit too: one interaction function, the same MFMA order in the deep layers.  total_logit is not
    # bit-equal (final_layer is two fmaf here, the tail's three-term DeepFM combine there): within tolerance.
    assert torch.equal(one[3], two[3])
    assert rankops.error_flags() == 0


def test_outside_the_fused_envelope_takes_more_than_one_launch():
    model, _ = model_for(TWELVE)
    assert not model.fused() and not rankops.common.fibinet_fits(12, 8, 4, "interaction", [512, 256, 128])
    assert rankops.common.fibinet_fits(6, 32, 2, "interaction", [512, 256, 128])
    cat = H.to_device(X.model_inputs(TWELVE), DEV)
    with torch.no_grad():
        model(cat)
        names = launches_of(lambda: model(cat))
    print(names)
    assert names[0] == "rk_fibinet_interaction" and len(names) > 1 and "rk_fibinet_forward" not in names
    with pytest.raises(RuntimeError, match="fused tail"):
        model.prepare(cat)


def test_out_of_range_id_reads_a_zero_row_and_raises_the_flag():
    model, params = model_for(WECHAT_300)
    cat = X.model_inputs(WECHAT_300)
    assert rankops.error_flags() == 0
    cat["feedid"][5] = model.vocab_sizes["feedid"]  # one past the last row
    zero_row = dict(params)  # the restatement over tables with a zero row appended at that index
    for k in ("first_order_embeddings.feedid.weight", "second_order_embeddings.feedid.weight"):
        zero_row[k] = torch.cat([params[k], torch.zeros_like(params[k][:1])])
    ref = X.forward(zero_row, cat)
    for two in (False, True):
        model.two_launch = two
        try:
            with torch.no_grad():
                out = model(H.to_device(cat, DEV))
        finally:
            model.two_launch = None
        assert rankops.error_flags() == _lib.RK_FLAG_INDEX_OOB
        check_outputs(out, ref, WECHAT_300[3])
        assert rankops.error_flags() == 0


def test_prepare_is_bit_equal_follows_its_inputs_and_replays_in_a_graph():
    model, _ = model_for(WECHAT_300)
    first = X.model_inputs(WECHAT_300)
    cat = H.to_device(first, DEV)
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
    # captured once, replayed after the inputs change back
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run_graph = model.prepare(cat)  # (bound to the capturing stream)
        captured = run_graph()
    for k in cat:
        cat[k].copy_(first[k])
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, want))
    assert rankops.error_flags() == 0


def test_prepare_of_the_two_launch_path_and_train_mode():
    model = X.build_model(WECHAT_300).to(DEV)
    cat = H.to_device(X.model_inputs(WECHAT_300), DEV)
    model.two_launch = True
    with torch.no_grad():
        want = model(cat)
    run = model.prepare(cat)
    assert all(torch.equal(a, b) for a, b in zip(run(), want))
    empty = model({k: v[:0] for k, v in cat.items()})
    assert len(empty) == 4 and all(o.shape == (0, 1) for o in empty)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        model(X.model_inputs(WECHAT_300))
    with pytest.raises(RuntimeError, match="eval mode"):
        model.train().prepare(cat)
    with pytest.raises(NotImplementedError):
        model(cat)
    assert rankops.error_flags() == 0


def test_a_batch_past_one_workgroup_per_cu_takes_the_two_launches():
    """forward takes the faster path at each batch size: the one launch up to one 16-sample workgroup per CU."""
    model, params = model_for(WECHAT_300)
    B = 16 * rankops.common._num_cus(torch.device(DEV)) + 1
    assert model.fused(B - 1, torch.device(DEV)) and not model.fused(B, torch.device(DEV))
    case = ("past", None, 8, B, "interaction", {})
    cat = X.model_inputs(case)
    dcat = H.to_device(cat, DEV)
    with torch.no_grad():
        out = model(dcat)
        names = launches_of(lambda: model(dcat))
        model.two_launch = False
        try:
            one = model(dcat)
            forced = launches_of(lambda: model(dcat))
        finally:
            model.two_launch = None
    print(names, forced)
    assert names[0] == "rk_fibinet_interaction" and len(names) > 1 and forced == ["rk_fibinet_forward"]
    ref = X.forward(params, cat)
    check_outputs(out, ref, B)
    check_outputs(one, ref, B)
    assert rankops.error_flags() == 0
