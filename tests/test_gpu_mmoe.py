"""GPU tests of MMoE: rk_mmoe_forward at op level (a dense segment, through rankops.mmoe), its raw C ABI
envelope, and rankops.MMoE at model level, against the float64 restatement in tests/mmoe_ref.py with
the tolerances derived there (50 x the restatement's own float32 drift)."""
import ctypes
import functools

import pytest
import torch

import helpers as H
import mmoe_ref as R
import rankops
from rankops import _lib, common, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_IDS = [c[0] for c in R.OP_CASES]
NAMES = ("mixed", "gate_probs", "logits", "probs")


def close(got, ref, tol, what):
    err = R.rel_err(got.detach(), ref)
    print(f"{what}: err {err:.3g} (tol {tol:.3g})")
    assert bool(torch.isfinite(got).all()), what
    assert err <= tol, (what, err, tol)


def on_gpu(obj):
    if isinstance(obj, (list, tuple)):
        return type(obj)(on_gpu(o) for o in obj)
    return obj.to(DEV) if isinstance(obj, torch.Tensor) else obj


def run_op(c, rows_slice=None, with_towers=True, bias=True):
    width = c[1]
    rows, experts, gates, towers = on_gpu(R.op_inputs(c))
    assert rows.stride(0) == width + R.ROW_PAD  # a row stride larger than the width
    x = rows[:, :width]
    if rows_slice is not None:
        x = x[rows_slice]
    if not bias:
        experts = [[(W, None) for W, _ in layers] for layers in experts]
        gates = [(W, None) for W, _ in gates]
    return rankops.mmoe(x, experts, gates, towers if with_towers else None)


@pytest.mark.parametrize("c", R.OP_CASES, ids=CASE_IDS)
def test_op_matches_restatement(c):
    name, width, E, K, eu, tu, B = c
    out = run_op(c)
    ref = R.op_reference(c)
    assert [tuple(t.shape) for t in out] == [(B, K, eu[-1]), (B, K, E), (B, K), (B, K)]
    for got, want, tol, what in zip(out, ref, R.tolerances(name), NAMES):
        close(got, want, tol, f"{name} {what}")
    again = run_op(c)
    assert all(torch.equal(a, b) for a, b in zip(out, again))  # fixed summation order
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("name", ["tile_edge", "odd"])
def test_rows_do_not_depend_on_their_batch(name):
    c = R.case(name)
    whole = run_op(c)
    first = run_op(c, rows_slice=slice(0, 16))
    for a, b, what in zip(first, whole, NAMES):
        assert a.shape[0] == 16 and torch.equal(a, b[:16]), what


def test_without_towers_and_without_biases():
    c = R.case("odd")
    full = run_op(c)
    two = run_op(c, with_towers=False)
    assert len(two) == 2 and torch.equal(two[0], full[0]) and torch.equal(two[1], full[1])
    # biases passed as None behave as zeros
    width = c[1]
    rows, experts, gates, towers = on_gpu(R.op_inputs(c))
    x = rows[:, :width]
    none = run_op(c, bias=False)
    zeros = rankops.mmoe(x, [[(W, torch.zeros_like(b)) for W, b in layers] for layers in experts],
                         [(W, torch.zeros_like(b)) for W, b in gates], towers)
    assert all(torch.equal(a, b) for a, b in zip(none, zeros))
    assert not torch.equal(none[0], full[0])
    ref = R.mmoe(rows[:, :width].double().cpu(), [[(W.double().cpu(), None) for W, _ in l] for l in experts],
                 [(W.double().cpu(), None) for W, _ in gates], R.cast(on_cpu(towers), torch.float64))
    for got, want, tol, what in zip(none, ref, R.tolerances("odd"), NAMES):
        close(got, want, tol, f"no bias {what}")
    empty = rankops.mmoe(x[:0], experts, gates, towers)
    assert [tuple(t.shape) for t in empty] == [(0, 2, 24), (0, 2, 3), (0, 2), (0, 2)]


def on_cpu(obj):
    if isinstance(obj, (list, tuple)):
        return type(obj)(on_cpu(o) for o in obj)
    return obj.cpu() if isinstance(obj, torch.Tensor) else obj


# ---------------------------------------------------------------- the raw C ABI

SENTINEL = -7.5


def raw_call(width=20, E=2, K=2, eu=(16,), tu=(8,), B=4, batch=None, null_segments=False):
    """rk_mmoe_forward on zero weights sized for the shape; returns (code, the four sentinel-filled
    outputs)."""
    lib = _lib.load()
    _lib.ensure_device(torch.device(DEV))
    img = lambda n, k: torch.zeros((n + 63) // 64 * 64, (k + 63) // 64 * 64, device=DEV)  # noqa: E731
    bufs = []

    def stacks(count, k_in, units):
        arr = (_lib.MmoeLayer * max(1, count * len(units)))()
        for s in range(count):
            k = k_in
            for l, n in enumerate(units):
                w, b = img(n, k), torch.zeros(n, device=DEV)
                bufs.extend([w, b])
                d = arr[s * len(units) + l]
                d.w, d.bias, d.n, d.act = w.data_ptr(), b.data_ptr(), n, _lib.RK_ACT_RELU
                k = n
        return arr
    x = torch.ones(max(B, 1), width, device=DEV)
    chunks = [ops.dense_segment(x, min(128, width - c), c, c) for c in range(0, width, 128)]  # <= 255 columns each
    segs = (_lib.Segment * len(chunks))(*chunks)
    ex = stacks(E, width, eu)
    tw = stacks(K, eu[-1], tu)
    gate = img(K * E, width)
    last = tu[-1] if tu else eu[-1]
    hw = [torch.zeros(last, device=DEV) for _ in range(K)]
    hb = [torch.zeros(1, device=DEV) for _ in range(K)]
    hwp = (ctypes.c_void_p * K)(*[t.data_ptr() for t in hw])
    hbp = (ctypes.c_void_p * K)(*[t.data_ptr() for t in hb])
    n = max(B, 1)
    out = [torch.full(shape, SENTINEL, device=DEV) for shape in ((n, K, eu[-1]), (n, K, E), (n, K), (n, K))]
    rc = lib.rk_mmoe_forward(None if null_segments else segs, len(chunks), width, B if batch is None else batch,
                             ex, E, len(eu), gate.data_ptr(), None, K, tw if tu else None, len(tu), hwp, hbp,
                             out[2].data_ptr(), out[3].data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                             _lib.raw_stream(DEV))
    torch.cuda.synchronize()
    return rc, out


def untouched(out):
    return all(bool((t == SENTINEL).all()) for t in out)


def test_envelope_and_argument_errors():
    rc, out = raw_call()
    assert rc == _lib.RK_OK, _lib.last_error()
    # zero weights: uniform gates, zero mixtures, zero logits
    assert bool((out[1] == 0.5).all()) and bool((out[0] == 0).all()) and bool((out[2] == 0).all())
    assert float((out[3] - 0.5).abs().max()) < 1e-6 and rankops.error_flags() == 0
    unsupported = [dict(E=17, K=1), dict(E=13, K=5), dict(width=257), dict(eu=(513,)), dict(tu=(513,)),
                   dict(eu=(8, 8, 8, 8))]
    for kw in unsupported:
        rc, out = raw_call(**kw)
        assert rc == _lib.RK_ERR_UNSUPPORTED, (kw, rc, _lib.last_error())
        assert "rk_mmoe_forward" in _lib.last_error() and untouched(out), kw
    for kw in (dict(null_segments=True), dict(batch=-1)):
        rc, out = raw_call(**kw)
        assert rc == 1, (kw, rc)  # RK_ERR_INVALID
        assert "rk_mmoe_forward" in _lib.last_error() and untouched(out), kw
    rc, out = raw_call(batch=0)
    assert rc == _lib.RK_OK and untouched(out)
    rc, _ = raw_call(E=16, K=4, width=256, eu=(512, 512, 512), tu=(512, 512, 512), B=3)  # the envelope's corner
    assert rc == _lib.RK_OK, _lib.last_error()


# ---------------------------------------------------------------- the model

@functools.lru_cache(maxsize=None)
def gpu_model(name):
    mc = next(m for m in R.MODEL_CASES if m[0] == name)
    cpu = R.build_model(mc)
    ref = R.forward(R.floats(H.cpu_params(cpu), torch.float64), **R.model_inputs(mc))
    return cpu.to(DEV), H.to_device(R.model_inputs(mc), DEV), ref


def check_model(out, ref, what):
    close(out[0], ref[0], R.PROB_TOL, f"{what} probabilities")
    close(out[1], ref[1], R.LOGIT_TOL, f"{what} logits")


@pytest.mark.parametrize("name", [m[0] for m in R.MODEL_CASES])
def test_model_matches_restatement(name):
    model, inp, ref = gpu_model(name)
    B, K = inp["dense"].shape[0], len(model.task_names)
    with torch.no_grad():
        out = model(inp["dense"], inp["category"])
        assert out[0].shape == out[1].shape == (B, K)
        check_model(out, ref, name)
        entries = len(model._eager)
        cached = model(inp["dense"], inp["category"])  # the EagerCalls hit
        assert len(model._eager) == entries
        common.EAGER_CACHE = False
        try:
            uncached = model(inp["dense"], inp["category"])
        finally:
            common.EAGER_CACHE = True
    for a, b, c in zip(out, cached, uncached):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert rankops.error_flags() == 0


def test_converted_and_strided_indices_agree():
    model, inp, ref = gpu_model("small_default")
    B = inp["dense"].shape[0]
    with torch.no_grad():
        want = model(inp["dense"], inp["category"])
        as32 = {k: v.to(torch.int32) for k, v in inp["category"].items()}
        strided = {}
        for k, v in inp["category"].items():
            buf = torch.zeros(B, 3, dtype=torch.int64, device=DEV)
            buf[:, 1] = v
            strided[k] = buf[:, 1]
            assert not strided[k].is_contiguous()
        for cat in (as32, strided):
            got = model(inp["dense"], cat)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_out_of_range_id_zeroes_the_field_and_raises_the_flag():
    model, inp, _ = gpu_model("small_default")
    mc = R.MODEL_CASES[0]
    cat = {k: v.clone() for k, v in inp["category"].items()}
    rows_of = model.embeddings["authorid"].num_embeddings
    cat["authorid"][5] = rows_of
    cat["authorid"][200] = -1
    keep = torch.ones(inp["dense"].shape[0])
    keep[5] = keep[200] = 0
    p = R.floats(H.cpu_params(model), torch.float64)
    ref = R.forward(p, inp["dense"].cpu(), H.to_device(cat, "cpu"), keep={"authorid": keep})
    with torch.no_grad():
        out = model(inp["dense"], cat)
    assert rankops.error_flags() == _lib.RK_FLAG_INDEX_OOB
    check_model(out, ref, "out-of-range id")
    assert rankops.error_flags() == 0


def test_prepare_is_bit_equal_follows_its_inputs_and_replays_in_a_graph():
    model, inp, ref = gpu_model("small_default")
    dense = inp["dense"].clone()
    cat = {k: v.clone() for k, v in inp["category"].items()}
    with torch.no_grad():
        want = model(dense, cat)
        run = model.prepare(dense, cat)
        first = run()
        assert torch.equal(first[0], want[0]) and torch.equal(first[1], want[1])
        second = run()
        assert all(a is b for a, b in zip(first, second))  # the same tensors on each call
        check_model(second, ref, "prepared")
        # in-place changes of the bound inputs are followed
        other = H.to_device(R.model_inputs(("x", "small", dense.shape[0], {}), seed=77), DEV)
        dense.copy_(other["dense"])
        for k in cat:
            cat[k].copy_(other["category"][k])
        moved = model(dense, cat)
        assert not torch.equal(moved[1], want[1])
        got = run()
        assert torch.equal(got[0], moved[0]) and torch.equal(got[1], moved[1])
        # captured once (a single chain of one kernel node) and replayed after the inputs change
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run_graph = model.prepare(dense, cat)
            captured = run_graph()
        dense.copy_(inp["dense"])
        for k in cat:
            cat[k].copy_(inp["category"][k])
        graph.replay()
        torch.cuda.synchronize()
        fresh = model(dense, cat)
        assert torch.equal(captured[0], fresh[0]) and torch.equal(captured[1], fresh[1])
        assert torch.equal(fresh[1], want[1])
    model.train()
    try:
        with pytest.raises(RuntimeError, match="eval mode"):
            model.prepare(dense, cat)
    finally:
        model.eval()
    assert rankops.error_flags() == 0


def test_forward_follows_an_in_place_weight_update():
    mc = R.MODEL_CASES[0]
    model = R.build_model(mc, seed=7).to(DEV)
    inp = H.to_device(R.model_inputs(mc), DEV)
    with torch.no_grad():
        before = model(inp["dense"], inp["category"])
        model.experts[1][0].weight.mul_(1.01)
        model.gates[2].weight.mul_(1.01)
        after = model(inp["dense"], inp["category"])
    assert not torch.equal(before[1], after[1])
    ref = R.forward(R.floats(H.cpu_params(model), torch.float64), **R.model_inputs(mc))
    check_model(after, ref, "after the update")


def test_eval_accumulators_take_the_strided_task_columns():
    model, inp, _ = gpu_model("small_default")
    B, K = inp["dense"].shape[0], len(model.task_names)
    g = torch.Generator().manual_seed(3)
    labels = (torch.rand(B, K, generator=g) < 0.4).float().to(DEV)
    with torch.no_grad():
        probs, logits = model(inp["dense"], inp["category"])
    for k in range(K):
        acc = rankops.EvalAccumulator(DEV)
        assert not probs[:, k].is_contiguous() or K == 1
        acc.add(probs[:, k], labels[:, k], logits[:, k])
        _, _, auc = acc.result()
        want = float(rankops.roc_auc(probs[:, k].contiguous(), labels[:, k].contiguous()))
        assert auc == want and 0.0 <= auc <= 1.0


def test_empty_batch_train_mode_and_cpu_tensors():
    model, inp, _ = gpu_model("small_default")
    empty = model(inp["dense"][:0], {k: v[:0] for k, v in inp["category"].items()})
    assert [tuple(t.shape) for t in empty] == [(0, 3), (0, 3)] and all(t.device.type == "cuda" for t in empty)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        model(inp["dense"].cpu(), inp["category"])
    model.train()
    try:
        with pytest.raises(NotImplementedError):
            model(inp["dense"], inp["category"])
    finally:
        model.eval()
