"""GPU tests of PLE: rk_ple_forward at op level (a dense segment, through rankops.ple), its raw C ABI
envelope, and rankops.PLE at model level, against the float64 restatement in tests/ple_ref.py with the
tolerances derived there (50 x the restatement's own float32 drift)."""
import functools

import pytest
import torch

import helpers as H
import mmoe_ref
import ple_ref as R
import rankops
from rankops import _lib, common, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_IDS = [c[0] for c in R.OP_CASES]
NAMES = ("representations", "gates", "logits", "probs")
MODEL_IDS = [m[0] for m in R.MODEL_CASES]


def close(got, ref, tol, what):
    err = R.rel_err(got.detach(), ref)
    print(f"{what}: err {err:.3g} (tol {tol:.3g})")
    assert bool(torch.isfinite(got).all()), what
    assert err <= tol, (what, err, tol)


def on_gpu(obj):
    if isinstance(obj, (list, tuple)):
        return type(obj)(on_gpu(o) for o in obj)
    return obj.to(DEV) if isinstance(obj, torch.Tensor) else obj


def on_cpu(obj):
    if isinstance(obj, (list, tuple)):
        return type(obj)(on_cpu(o) for o in obj)
    return obj.cpu() if isinstance(obj, torch.Tensor) else obj


def without_biases(levels, f=lambda b: None):
    return [([[[(W, f(b)) for W, b in e] for e in task] for task in sp], [[(W, f(b)) for W, b in e] for e in sh],
             [(W, f(b)) for W, b in gt], None if sg is None else (sg[0], f(sg[1]))) for sp, sh, gt, sg in levels]


def run_op(c, rows_slice=None, with_towers=True, return_levels=True):
    width = c[1]
    rows, levels, towers = on_gpu(R.op_inputs(c))
    assert rows.stride(0) == width + R.ROW_PAD  # a row stride larger than the width
    x = rows[:, :width]
    if rows_slice is not None:
        x = x[rows_slice]
    return rankops.ple(x, levels, towers if with_towers else None, return_levels=return_levels)


def as_ref(out):
    """rankops.ple(..., towers, return_levels=True)'s result in ple_ref.ple's order."""
    logits, probs, levels = out
    return levels, logits, probs


def tensors(out):
    """Every tensor of a (levels, logits, probs) result, flat."""
    return [t for group in R.flat(out) for t in group]


@pytest.mark.parametrize("c", R.OP_CASES, ids=CASE_IDS)
def test_op_matches_restatement(c):
    name, width, L, K, ms, mc, eu, tu, B = c
    out = as_ref(run_op(c))
    ref = R.op_reference(c)
    levels = out[0]
    assert [tuple(lv[0].shape) for lv in levels] == [(B, K + 1, eu[-1])] * (L - 1) + [(B, K, eu[-1])]
    assert all(tuple(lv[1].shape) == (B, K, ms + mc) for lv in levels)
    assert [None if lv[2] is None else tuple(lv[2].shape) for lv in levels] == [(B, K * ms + mc)] * (L - 1) + [None]
    assert out[1].shape == out[2].shape == (B, K)
    for got, want, tol, what in zip(R.flat(out), R.flat(ref), R.tolerances(name), NAMES):
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            close(g, w, tol, f"{name} {what} [{i}]")
    again = as_ref(run_op(c))
    assert all(torch.equal(a, b) for a, b in zip(tensors(out), tensors(again)))  # fixed summation order
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("name", ["tile_edge", "odd"])
def test_rows_do_not_depend_on_their_batch(name):
    c = R.case(name)
    whole = tensors(as_ref(run_op(c)))
    first = tensors(as_ref(run_op(c, rows_slice=slice(0, 16))))
    assert len(whole) == len(first)
    for a, b in zip(first, whole):
        assert a.shape[0] == 16 and torch.equal(a, b[:16])


def test_return_levels_towers_biases_and_the_empty_batch():
    c = R.case("odd")
    full = run_op(c)
    short = run_op(c, return_levels=False)
    assert len(short) == 2 and torch.equal(short[0], full[0]) and torch.equal(short[1], full[1])
    # without towers: representations and gates only
    bare = run_op(c, with_towers=False)
    assert len(bare) == len(full[2]) == 3
    assert all(torch.equal(a, b) for a, b in zip(tensors((bare, None, None)), tensors((full[2], None, None))))
    last = run_op(c, with_towers=False, return_levels=False)
    assert len(last) == 2 and torch.equal(last[0], full[2][-1][0]) and torch.equal(last[1], full[2][-1][1])
    # biases passed as None behave as zeros
    width = c[1]
    rows, levels, towers = on_gpu(R.op_inputs(c))
    x = rows[:, :width]
    none = as_ref(rankops.ple(x, without_biases(levels), towers, return_levels=True))
    zeros = as_ref(rankops.ple(x, without_biases(levels, torch.zeros_like), towers, return_levels=True))
    assert all(torch.equal(a, b) for a, b in zip(tensors(none), tensors(zeros)))
    assert not torch.equal(none[1], full[0])
    ref = R.ple(x.double().cpu(), without_biases(R.cast(on_cpu(levels), torch.float64)), R.cast(on_cpu(towers), torch.float64))
    for got, want, tol, what in zip(R.flat(none), R.flat(ref), R.tolerances("odd"), NAMES):
        for g, w in zip(got, want):
            close(g, w, tol, f"no bias {what}")
    logits, probs, lv = rankops.ple(x[:0], levels, towers, return_levels=True)
    assert tuple(logits.shape) == tuple(probs.shape) == (0, 2)
    assert [tuple(t[0].shape) for t in lv] == [(0, 3, 24), (0, 3, 24), (0, 2, 24)]
    assert [tuple(t[1].shape) for t in lv] == [(0, 2, 3)] * 3
    assert [None if t[2] is None else tuple(t[2].shape) for t in lv] == [(0, 5), (0, 5), None]


def test_one_level_without_task_experts_agrees_with_mmoe():
    c = R.case("mmoe_like")
    rows, levels, towers = on_gpu(R.op_inputs(c))
    x = rows[:, :c[1]]
    (_, experts, gates, _), = levels
    logits, probs = rankops.ple(x, levels, towers)
    _, _, mlogits, mprobs = rankops.mmoe(x, experts, gates, towers)
    # both are within their own tolerance of the same float64 function (test_ple_ref.py), so of each other
    # within the sum
    close(logits, mlogits.double().cpu(), R.LOGIT_TOL + mmoe_ref.LOGIT_TOL, "ple vs mmoe logits")
    close(probs, mprobs.double().cpu(), R.PROB_TOL + mmoe_ref.PROB_TOL, "ple vs mmoe probs")
    ref = R.op_reference(c)
    close(mlogits, ref[1], mmoe_ref.LOGIT_TOL, "mmoe logits vs the PLE restatement")


# ---------------------------------------------------------------- the raw C ABI

SENTINEL = -7.5


def raw_call(width=20, L=2, K=2, ms=1, mc=1, eu=(16,), tu=(8,), B=4, batch=None, null_segments=False, nseg=None,
             table_extra=0):
    """rk_ple_forward on zero weights sized for the shape; returns (code, [logits, probs, reps…, gates…],
    all sentinel-filled)."""
    lib = _lib.load()
    _lib.ensure_device(torch.device(DEV))
    img = lambda n, k: torch.zeros((n + 63) // 64 * 64, (k + 63) // 64 * 64, device=DEV)  # noqa: E731
    H_, NE = eu[-1], K * ms + mc
    entries = []
    for j in range(L):
        for _ in range(NE):
            k = width if j == 0 else H_
            for n in eu:
                entries.append((img(n, k), torch.zeros(n, device=DEV)))
                k = n
    for j in range(L):
        k = width if j == 0 else H_
        entries += [(img(ms + mc, k), None) for _ in range(K)] + [(img(NE, k), None)]
    for _ in range(K):
        k = H_
        for n in tu:
            entries.append((img(n, k), torch.zeros(n, device=DEV)))
            k = n
    last = tu[-1] if tu else H_
    entries += [(torch.zeros(last, device=DEV), torch.zeros(1, device=DEV)) for _ in range(K)]
    entries += entries[:1] * table_extra
    n = max(B, 1)
    x = torch.ones(n, width, device=DEV)
    if nseg is None:
        chunks = [ops.dense_segment(x, min(128, width - c), c, c) for c in range(0, width, 128)]  # <= 255 columns each
    else:
        chunks = [ops.dense_segment(x, 1, c, c) for c in range(nseg)]
    GT = ms + mc
    full = lambda shape: torch.full(shape, SENTINEL, device=DEV)  # noqa: E731
    logits, probs = full((n, K)), full((n, K))
    reps = [full((n, K + (j < L - 1), H_)) for j in range(L)]
    gates = [full((n, K * GT + (NE if j < L - 1 else 0))) for j in range(L)]
    args, keep = ops.ple_forward_args(chunks, width, B if batch is None else batch, L, K, ms, mc, list(eu), list(tu),
                                      entries, True, torch.device(DEV), logits=logits, probs=probs, reps=reps,
                                      gates=gates)
    if null_segments:
        args[0] = None
    args[-1] = _lib.raw_stream(DEV)
    rc = lib.rk_ple_forward(*args)
    torch.cuda.synchronize()
    return rc, [logits, probs] + reps + gates


def untouched(out):
    return all(bool((t == SENTINEL).all()) for t in out)


def test_envelope_and_argument_errors():
    rc, out = raw_call()
    assert rc == _lib.RK_OK, _lib.last_error()
    logits, probs, rep0, rep1, gate0, gate1 = out
    # zero weights: uniform gates (two columns per task gate, three for the shared one), zero logits
    assert bool((gate0[:, :4] == 0.5).all()) and float((gate0[:, 4:] - 1 / 3).abs().max()) < 1e-7
    assert bool((gate1 == 0.5).all()) and gate1.shape[1] == 4
    assert bool((rep0 == 0).all()) and bool((rep1 == 0).all()) and bool((logits == 0).all())
    assert float((probs - 0.5).abs().max()) < 1e-6 and rankops.error_flags() == 0
    unsupported = [dict(L=5), dict(K=9, ms=0), dict(K=8, ms=8, mc=1), dict(K=1, ms=0, mc=65), dict(width=257),
                   dict(nseg=17), dict(eu=(513,)), dict(tu=(513,)), dict(eu=(8, 8, 8, 8)), dict(tu=(8, 8, 8, 8)),
                   dict(width=200, K=1, mc=2, eu=(512, 384), tu=(512,))]  # the last: 175,488 B of LDS
    for kw in unsupported:
        rc, out = raw_call(**kw)
        assert rc == _lib.RK_ERR_UNSUPPORTED, (kw, rc, _lib.last_error())
        assert "rk_ple_forward" in _lib.last_error() and untouched(out), kw
    for kw in (dict(null_segments=True), dict(batch=-1), dict(table_extra=1), dict(L=0), dict(mc=0), dict(eu=(0,))):
        rc, out = raw_call(**kw)
        assert rc == 1, (kw, rc)  # RK_ERR_INVALID
        assert "rk_ple_forward" in _lib.last_error() and untouched(out), kw
    rc, out = raw_call(batch=0)
    assert rc == _lib.RK_OK and untouched(out)
    # the envelope's corners: the widest the LDS takes, the most levels / tasks / stacks, the deepest stacks
    for kw in (dict(width=200, K=1, mc=2, eu=(512, 320), tu=(512,), B=3),
               dict(width=50, L=4, K=8, ms=7, mc=8, eu=(16,), tu=(), B=3), dict(width=256, B=3),
               dict(width=50, L=1, K=1, ms=0, mc=64, eu=(8, 8, 8), tu=(8, 8, 8), B=17)):
        rc, out = raw_call(**kw)
        assert rc == _lib.RK_OK, (kw, _lib.last_error())
        assert bool((out[0] == 0).all()) and not any(bool((t == SENTINEL).any()) for t in out), kw
    assert rankops.error_flags() == 0


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


@pytest.mark.parametrize("name", MODEL_IDS)
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


@pytest.mark.parametrize("name", MODEL_IDS)
def test_converted_and_strided_indices_agree(name):
    model, inp, ref = gpu_model(name)
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


@pytest.mark.parametrize("name", MODEL_IDS)
def test_out_of_range_id_zeroes_the_field_and_raises_the_flag(name):
    model, inp, _ = gpu_model(name)
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


@pytest.mark.parametrize("name", MODEL_IDS)
def test_prepare_is_bit_equal_follows_its_inputs_and_replays_in_a_graph(name):
    model, inp, ref = gpu_model(name)
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
        which = next(m[1] for m in R.MODEL_CASES if m[0] == name)
        other = H.to_device(R.model_inputs(("x", which, dense.shape[0], {}), seed=77), DEV)
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


@pytest.mark.parametrize("mc", R.MODEL_CASES, ids=MODEL_IDS)
def test_forward_follows_an_in_place_weight_update(mc):
    model = R.build_model(mc, seed=7).to(DEV)
    inp = H.to_device(R.model_inputs(mc), DEV)
    ms = model.num_specific_experts
    with torch.no_grad():
        before = model(inp["dense"], inp["category"])
        model.levels[1].specific_experts[1][ms - 1][0].weight.mul_(1.01)
        mid = model(inp["dense"], inp["category"])
        model.levels[0].shared_gate.weight.mul_(1.05)
        after = model(inp["dense"], inp["category"])
    assert not torch.equal(before[1], mid[1]) and not torch.equal(mid[1], after[1])
    ref = R.forward(R.floats(H.cpu_params(model), torch.float64), **R.model_inputs(mc))
    check_model(after, ref, "after the update")


@pytest.mark.parametrize("name", MODEL_IDS)
def test_eval_accumulators_take_the_strided_task_columns(name):
    model, inp, _ = gpu_model(name)
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


@pytest.mark.parametrize("name", MODEL_IDS)
def test_empty_batch_train_mode_and_cpu_tensors(name):
    model, inp, _ = gpu_model(name)
    K = len(model.task_names)
    empty = model(inp["dense"][:0], {k: v[:0] for k, v in inp["category"].items()})
    assert [tuple(t.shape) for t in empty] == [(0, K), (0, K)] and all(t.device.type == "cuda" for t in empty)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        model(inp["dense"].cpu(), inp["category"])
    model.train()
    try:
        with pytest.raises(NotImplementedError):
            model(inp["dense"], inp["category"])
    finally:
        model.eval()
