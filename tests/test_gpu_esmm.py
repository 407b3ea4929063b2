"""GPU tests of ESMM: rk_esmm_forward at op level (a dense segment, through rankops.esmm), its raw C ABI
envelope, and rankops.ESMM at model level, against the float64 restatement in tests/esmm_ref.py with the
tolerances derived there (50 x the restatement's own float32 drift)."""
import ctypes
import functools

import pytest
import torch

import esmm_ref as R
import helpers as H
import rankops
from rankops import _lib, common, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_IDS = [c[0] for c in R.OP_CASES]
NAMES = ("probs", "logits", "cond")
INVALID = 1  # RK_ERR_INVALID (include/rankops.h)


def close(got, ref, tol, what):
    err = R.rel_err(got.detach(), ref)
    print(f"{what}: err {err:.3g} (tol {tol:.3g})")
    assert bool(torch.isfinite(got).all()), what
    assert got.shape == ref.shape and err <= tol, (what, err, tol)


def on_gpu(obj):
    if isinstance(obj, (list, tuple)):
        return type(obj)(on_gpu(o) for o in obj)
    return obj.to(DEV) if isinstance(obj, torch.Tensor) else obj


def on_cpu(obj):
    if isinstance(obj, (list, tuple)):
        return type(obj)(on_cpu(o) for o in obj)
    return obj.cpu() if isinstance(obj, torch.Tensor) else obj


def run_op(c, rows_slice=None, cond=True):
    width = c[1]
    rows, towers = on_gpu(R.op_inputs(c))
    assert rows.stride(0) == width + R.ROW_PAD  # a row stride larger than the width
    x = rows[:, :width]
    if rows_slice is not None:
        x = x[rows_slice]
    return rankops.esmm(x, towers, return_conditional=cond)


def tols(name):
    lt, pt, ct = R.tolerances(name)
    return pt, lt, ct  # in the order of the outputs


@pytest.mark.parametrize("c", R.OP_CASES, ids=CASE_IDS)
def test_op_matches_restatement(c):
    name, width, K, tu, B = c
    out = run_op(c)
    ref = R.op_reference(c)
    assert [tuple(t.shape) for t in out] == [(B, K)] * 3
    for got, want, tol, what in zip(out, ref, tols(name), NAMES):
        close(got, want, tol, f"{name} {what}")
    assert torch.equal(out[0][:, 0], out[2][:, 0])  # column 0 of the probabilities is sigmoid(logit_0)
    again = run_op(c)
    assert all(torch.equal(a, b) for a, b in zip(out, again))  # fixed summation order
    two = run_op(c, cond=False)
    assert len(two) == 2 and torch.equal(two[0], out[0]) and torch.equal(two[1], out[1])
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("name", ["tile_edge", "odd"])
def test_rows_do_not_depend_on_their_batch(name):
    c = R.case(name)
    whole = run_op(c)
    first = run_op(c, rows_slice=slice(0, 16))
    for a, b, what in zip(first, whole, NAMES):
        assert a.shape[0] == 16 and torch.equal(a, b[:16]), what
    # the same rows inside a larger batch, at other positions of their tiles
    rows, towers = on_gpu(R.op_inputs(c))
    x = rows[:, :c[1]]
    big = torch.cat([x[5:12], x, x[:3]], dim=0)
    inside = rankops.esmm(big, towers, return_conditional=True)
    for a, b, what in zip(inside, whole, NAMES):
        assert torch.equal(a[7:7 + c[4]], b), what


def test_missing_biases_and_empty_batch():
    c = R.case("odd")
    rows, towers = on_gpu(R.op_inputs(c))
    x = rows[:, :c[1]]
    full = run_op(c)
    nb = [([(W, None) for W, _ in hidden], (w, None)) for hidden, (w, _) in towers]
    zb = [([(W, torch.zeros_like(b)) for W, b in hidden], (w, torch.zeros_like(b2))) for hidden, (w, b2) in towers]
    none = rankops.esmm(x, nb, return_conditional=True)
    zeros = rankops.esmm(x, zb, return_conditional=True)
    assert all(torch.equal(a, b) for a, b in zip(none, zeros)) and not torch.equal(none[1], full[1])
    ref = R.esmm(x.double().cpu(), R.cast(on_cpu(nb), torch.float64))
    for got, want, tol, what in zip(none, ref, tols("odd"), NAMES):
        close(got, want, tol, f"no bias {what}")
    empty = rankops.esmm(x[:0], towers, return_conditional=True)
    assert [tuple(t.shape) for t in empty] == [(0, 3)] * 3
    with pytest.raises(rankops.RankOpsError, match="rk_esmm_forward"):
        rankops.esmm(x, towers[:1])  # one tower is no chain


# ---------------------------------------------------------------- the raw C ABI

SENTINEL = -7.5


def raw_call(width=20, K=2, tu=(16,), B=4, batch=None, null_segments=False, outputs=(0, 1, 2), misalign=False):
    """rk_esmm_forward on zero weights sized for the shape; returns (code, the three sentinel-filled outputs
    (logits, probs, cond)); `outputs`: which of them are passed."""
    lib = _lib.load()
    _lib.ensure_device(torch.device(DEV))
    bufs = []
    arr = (_lib.MmoeLayer * max(1, K * len(tu)))()
    for k in range(K):
        kin = width
        for l, n in enumerate(tu):
            w = torch.zeros((n + 63) // 64 * 64, (kin + 63) // 64 * 64 + 4, device=DEV)
            b = torch.zeros(n, device=DEV)
            bufs.extend([w, b])
            d = arr[k * len(tu) + l]
            d.w, d.bias, d.n, d.act = w.data_ptr() + (4 if misalign else 0), b.data_ptr(), n, _lib.RK_ACT_RELU
            kin = n
    x = torch.ones(max(B, 1), min(width, 512), device=DEV)
    chunks = [ops.dense_segment(x, min(128, x.shape[1] - c), c, c) for c in range(0, x.shape[1], 128)]
    segs = (_lib.Segment * len(chunks))(*chunks)
    last = tu[-1] if tu else width
    hw = [torch.zeros(last, device=DEV) for _ in range(K)]
    hb = [torch.zeros(1, device=DEV) for _ in range(K)]
    hwp = (ctypes.c_void_p * K)(*[t.data_ptr() for t in hw])
    hbp = (ctypes.c_void_p * K)(*[t.data_ptr() for t in hb])
    out = [torch.full((max(B, 1), K), SENTINEL, device=DEV) for _ in range(3)]
    ptrs = [out[i].data_ptr() if i in outputs else None for i in range(3)]
    rc = lib.rk_esmm_forward(None if null_segments else segs, len(chunks), width, B if batch is None else batch, arr, K,
                             len(tu), hwp, hbp, ptrs[0], ptrs[1], ptrs[2], _lib.raw_stream(DEV))
    torch.cuda.synchronize()
    return rc, out


def untouched(out):
    return all(bool((t == SENTINEL).all()) for t in out)


def test_envelope_and_argument_errors():
    rc, out = raw_call()
    assert rc == _lib.RK_OK, _lib.last_error()
    # zero weights: zero logits, conditionals 1/2, probabilities 1/2 and 1/4
    assert bool((out[0] == 0).all()) and float((out[2] - 0.5).abs().max()) < 1e-6
    assert float((out[1][:, 0] - 0.5).abs().max()) < 1e-6 and float((out[1][:, 1] - 0.25).abs().max()) < 1e-6
    assert rankops.error_flags() == 0
    for kw in (dict(K=1), dict(K=9), dict(tu=()), dict(tu=(8, 8, 8, 8)), dict(width=513), dict(tu=(513,))):
        rc, out = raw_call(**kw)
        assert rc == _lib.RK_ERR_UNSUPPORTED, (kw, rc, _lib.last_error())
        assert "rk_esmm_forward" in _lib.last_error() and untouched(out), kw
    for kw in (dict(null_segments=True), dict(batch=-1), dict(outputs=()), dict(misalign=True)):
        rc, out = raw_call(**kw)
        assert rc == INVALID, (kw, rc)
        assert "rk_esmm_forward" in _lib.last_error() and untouched(out), kw
    rc, out = raw_call(batch=0)
    assert rc == _lib.RK_OK and untouched(out)
    full = raw_call(B=20)[1]
    for i in range(3):  # each output requested alone
        rc, out = raw_call(B=20, outputs=(i,))
        assert rc == _lib.RK_OK and torch.equal(out[i], full[i])
        assert all(bool((out[j] == SENTINEL).all()) for j in range(3) if j != i)
    rc, _ = raw_call(K=8, width=256, tu=(512, 512, 512), B=3)  # the envelope's corner
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
        assert torch.equal(a, b) and torch.equal(a, c)  # two runs give equal bits
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
        # the bound forward is one launch: one kernel node when captured
        bound = model._build(dense, list(model.embeddings), [cat[n] for n in model.embeddings], pin=True)
        assert [name for name, _ in bound.launches] == ["rk_esmm_forward"]
        # in-place changes of the bound inputs are followed
        other = H.to_device(R.model_inputs(("x", "small", dense.shape[0], {}), seed=77), DEV)
        dense.copy_(other["dense"])
        for k in cat:
            cat[k].copy_(other["category"][k])
        moved = model(dense, cat)
        assert not torch.equal(moved[1], want[1])
        got = run()
        assert torch.equal(got[0], moved[0]) and torch.equal(got[1], moved[1])
        # captured once and replayed after the inputs change
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
        model.towers[1][0].weight.mul_(1.01)
        model.tower_outputs[0].weight.mul_(1.01)
        after = model(inp["dense"], inp["category"])
    assert not torch.equal(before[1][:, 0], after[1][:, 0]) and not torch.equal(before[1][:, 1], after[1][:, 1])
    ref = R.forward(R.floats(H.cpu_params(model), torch.float64), **R.model_inputs(mc))
    check_model(after, ref, "after the update")


def test_eval_accumulators_take_the_strided_task_columns():
    model, inp, _ = gpu_model("small_alt")
    B, K = inp["dense"].shape[0], len(model.task_names)
    g = torch.Generator().manual_seed(3)
    labels = torch.cumprod((torch.rand(B, K, generator=g) < 0.6).float(), dim=1).to(DEV)
    with torch.no_grad():
        probs, logits = model(inp["dense"], inp["category"])
    for k in range(K):
        acc = rankops.EvalAccumulator(DEV)
        assert not probs[:, k].is_contiguous()
        joint = torch.logit(probs[:, k].double()).float()  # the joint probability's own logit
        acc.add(probs[:, k], labels[:, k], joint)
        _, _, auc = acc.result()
        want = float(rankops.roc_auc(probs[:, k].contiguous(), labels[:, k].contiguous()))
        assert auc == want and 0.0 <= auc <= 1.0


def test_empty_batch_train_mode_and_cpu_tensors():
    model, inp, _ = gpu_model("small_default")
    empty = model(inp["dense"][:0], {k: v[:0] for k, v in inp["category"].items()})
    assert [tuple(t.shape) for t in empty] == [(0, 2), (0, 2)] and all(t.device.type == "cuda" for t in empty)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        model(inp["dense"].cpu(), inp["category"])
    model.train()
    try:
        with pytest.raises(NotImplementedError):
            model(inp["dense"], inp["category"])
    finally:
        model.eval()
