"""GPU tests of rk_dien_interest / rk_dien_interest_dense and rankops.DIEN against the float64
restatement tests/dien_ref.py.

Tolerances (not tuned on the kernel): the recurrence evaluated in fp32 stays within 2e-7 of the
fp64 one with the draws used here (weights uniform(-0.5, 0.5), gate biases 1 + that, N(0,1) keys
and queries; B 256, T 50, four seeds, both cells), so the op-level bound is atol 1e-5, rtol 0 — 50
times that drift, room for hardware exp / rcp and another summation order, while a swapped gate,
a missed mask or an off-by-one step shows at 1e-2.  Model outputs use the project's 1e-4 / 1e-4."""
import functools

import pytest
import torch

import dien_ref
import helpers as H
import rankops
from rankops import _lib, ops

pytestmark = pytest.mark.gpu

CELLS = ("AGRU", "AUGRU")
SHAPES = [(1, 1, 16, 8), (3, 3, 8, 8), (67, 50, 16, 8), (5, 200, 32, 16), (64, 50, 16, 16)]
OP_TOL = dict(atol=1e-5, rtol=0)
VOCAB = 301


@functools.lru_cache(maxsize=None)
def case(B, T, Hd, nh, seed=11):
    """Seeded op inputs (CPU), shared by every test of the shape and never modified."""
    g = torch.Generator().manual_seed(seed + 13 * B + T)
    q = torch.randn(B, Hd, generator=g)
    table = torch.randn(VOCAB, Hd, generator=g)
    ids = torch.randint(0, VOCAB, (B, T), generator=g)
    lens = torch.randint(0, T + 1, (B,), generator=g)
    forced = torch.tensor([0, 1, T])[:B] if B >= 3 else torch.tensor([T])[:B]
    lens[:len(forced)] = forced
    return q, table, ids, lens, tuple(dien_ref.draw_weights(Hd, nh, seed + 1))


@functools.lru_cache(maxsize=None)
def reference(B, T, Hd, nh, cell):
    q, table, ids, lens, w = case(B, T, Hd, nh)
    s, a, _ = dien_ref.interest(q, table[ids], lens, w, cell)
    return s, a


def cuda(*ts):
    return [t.cuda() if isinstance(t, torch.Tensor) else [x.cuda() for x in t] for t in ts]


def report(name, got, want):
    err = (got.double().cpu() - want).abs().max().item() if want.numel() else 0.0
    print(f"{name}: max |err| = {err:.3e}")


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dense_op_matches_restatement(shape, cell):
    q, table, ids, lens, w = case(*shape)
    want_s, want_a = reference(*shape, cell)
    dq, dk, dl, dw = cuda(q, table[ids], lens, w)
    s, a = rankops.dien_interest(dq, dk, dl, dw, cell, return_attention=True)
    torch.cuda.synchronize()
    report(f"state {shape} {cell}", s, want_s)
    report(f"attention {shape} {cell}", a, want_a)
    assert s.shape == (shape[0], shape[3]) and a.shape == shape[:2] and s.dtype == torch.float32
    torch.testing.assert_close(s.double().cpu(), want_s, **OP_TOL)
    torch.testing.assert_close(a.double().cpu(), want_a, **OP_TOL)
    zero = lens == 0
    assert torch.equal(s.cpu()[zero], torch.zeros(int(zero.sum()), shape[3]))
    only = rankops.dien_interest(dq, dk, dl, dw, cell)  # without the attention output
    assert torch.equal(only, s)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gather_op_is_bit_equal_to_dense_op(shape, cell):
    q, table, ids, lens, w = case(*shape)
    dq, dt, di, dl, dw = cuda(q, table, ids, lens, w)
    s0, a0 = rankops.dien_interest(dq, dt[di], dl, dw, cell, return_attention=True)
    s1, a1 = rankops.dien_interest_gather(dq, dt, di, dl, dw, cell, return_attention=True)
    assert torch.equal(s0, s1) and torch.equal(a0, a1)
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("cell", CELLS)
def test_ids_past_the_length_are_never_read(cell):
    shape = (67, 50, 16, 8)
    q, table, ids, lens, w = case(*shape)
    dq, dt, dl, dw = cuda(q, table, lens, w)
    base = rankops.dien_interest_gather(dq, dt, ids.cuda(), dl, dw, cell, return_attention=True)
    past = torch.arange(shape[1])[None, :] >= lens[:, None]
    for poison in (VOCAB - 1, VOCAB + 5, -1, 2 ** 40):
        bad = ids.clone()
        bad[past] = poison
        got = rankops.dien_interest_gather(dq, dt, bad.cuda(), dl, dw, cell, return_attention=True)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), poison
        assert rankops.error_flags() == 0, poison


def test_out_of_range_id_reads_a_zero_row_and_raises_the_flag():
    shape = (67, 50, 16, 8)
    q, table, ids, lens, w = case(*shape)
    b = int(torch.nonzero(lens >= 5)[0])
    bad = ids.clone()
    bad[b, 3] = VOCAB  # one past the last row, at t = 3 < len
    keys = table[ids].clone()
    keys[b, 3] = 0.0
    want_s, want_a, _ = dien_ref.interest(q, keys, lens, w, "AUGRU")
    dq, dt, dl, dw = cuda(q, table, lens, w)
    assert rankops.error_flags() == 0
    s, a = rankops.dien_interest_gather(dq, dt, bad.cuda(), dl, dw, "AUGRU", return_attention=True)
    flags = rankops.error_flags()  # reads and resets
    assert flags & _lib.RK_FLAG_INDEX_OOB
    assert rankops.error_flags() == 0
    torch.testing.assert_close(s.double().cpu(), want_s, **OP_TOL)
    torch.testing.assert_close(a.double().cpu(), want_a, **OP_TOL)
    clean = reference(*shape, "AUGRU")[0]
    assert (want_s[b] - clean[b]).abs().max() > 1e-4  # the zero row does change this sample


@pytest.mark.parametrize("cell", CELLS)
def test_strided_query_and_output_in_one_row(cell):
    shape = (67, 50, 16, 8)
    B, T, Hd, nh = shape
    q, table, ids, lens, w = case(*shape)
    dt, di, dl, dw = cuda(table, ids, lens, w)
    width, q_col = 3 + Hd + 5 + nh, 3  # [3 | query | 5 | state]: the query is not 16-B aligned
    row = torch.full((B, width), 777.0, device="cuda")
    row[:, q_col:q_col + Hd] = q.cuda()
    before = row.clone()
    ops.dien_interest(_lib.fptr(row, q_col), width, dt, di, dl, T, Hd, nh, ops.DIEN_CELLS[cell], dw,
                      _lib.fptr(row, width - nh), width, None, B, row.device)
    torch.cuda.synchronize()
    assert torch.equal(row[:, :width - nh], before[:, :width - nh])
    torch.testing.assert_close(row[:, width - nh:].double().cpu(), reference(*shape, cell)[0], **OP_TOL)
    dense = rankops.dien_interest(q.cuda(), dt[di], dl, dw, cell)
    assert torch.equal(row[:, width - nh:], dense)


@pytest.mark.parametrize("shape", [(67, 50, 16, 8), (5, 200, 32, 16)], ids=lambda s: "x".join(map(str, s)))
def test_two_launches_are_bit_equal(shape):
    q, table, ids, lens, w = case(*shape)
    dq, dt, di, dl, dw = cuda(q, table, ids, lens, w)
    for cell in CELLS:
        a = rankops.dien_interest_gather(dq, dt, di, dl, dw, cell, return_attention=True)
        b = rankops.dien_interest_gather(dq, dt, di, dl, dw, cell, return_attention=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("B,T,Hd,nh", [(2, 3, 12, 8), (2, 3, 16, 4), (2, 257, 16, 8)])
def test_outside_the_envelope_is_not_implemented(B, T, Hd, nh):
    g = torch.Generator().manual_seed(0)
    q, k = torch.randn(B, Hd, generator=g).cuda(), torch.randn(B, T, Hd, generator=g).cuda()
    lens = torch.full((B,), T).cuda()
    w = [x.cuda() for x in dien_ref.draw_weights(Hd, nh, 0)]
    with pytest.raises(NotImplementedError, match="envelope"):
        rankops.dien_interest(q, k, lens, w)
    with pytest.raises(NotImplementedError, match="envelope"):
        rankops.dien_interest_gather(q, torch.randn(9, Hd, generator=g).cuda(), torch.zeros(B, T, dtype=torch.int64,
                                                                                            device="cuda"), lens, w)
    out = torch.empty(B, nh, device="cuda")
    with pytest.raises(rankops.RankOpsError) as e:  # the C entry point itself refuses, before any launch
        ops.dien_interest_dense(q, k, lens, nh, 0, w, out, None)
    assert e.value.code == _lib.RK_ERR_UNSUPPORTED


def test_bad_arguments_are_value_errors():
    q, table, ids, lens, w = case(3, 3, 8, 8)
    dq, dk, dl, dw = cuda(q, table[ids], lens, w)
    with pytest.raises(ValueError):
        rankops.dien_interest(dq, dk, dl, dw, "GRU")
    with pytest.raises(ValueError):
        rankops.dien_interest(dq, dk, dl, dw[:8])
    with pytest.raises(ValueError):
        rankops.dien_interest(dq[:2], dk, dl, dw)
    with pytest.raises(ValueError):
        rankops.dien_interest(dq, dk, dl[:2], dw)
    empty = rankops.dien_interest(dq[:0], dk[:0], dl[:0], dw, return_attention=True)
    assert empty[0].shape == (0, 8) and empty[1].shape == (0, 3)


# ------------------------------------------------------------------ the module

def model_and_inputs(cell="AGRU", activation="dice", batch_norm=True, B=64, T=50, seed=42):
    torch.manual_seed(seed)
    m = rankops.DIEN(None, activation=activation, batch_norm=batch_norm, custom_gru_type=cell,
                     vocab_sizes=H.SMALL_VOCAB)
    H.randomize_eval_stats(m, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():  # gate biases away from 1, candidate biases away from 0
        for cellm in (m.gru, m.evolution):
            for lin in cellm.values():
                lin.bias.add_(0.5 * (torch.rand(lin.bias.shape, generator=g) - 0.5))
    inp = H.din_inputs(B, T, H.SMALL_VOCAB, seed=seed + 3)
    lens = inp["sequence"][dien_ref.SEQ_KEY + "_length"]
    if B >= 3:
        lens[:3] = torch.tensor([0, 1, T])
    return m.eval(), inp


def call(m, inp, **kw):
    return m(inp["dense"], inp["category"], inp["sequence"], inp["target"], **kw)


def ref_forward(m, inp, cell, activation, batch_norm):
    return dien_ref.forward(H.cpu_params(m), inp["dense"], inp["category"], inp["sequence"], inp["target"],
                            activation=activation, batch_norm=batch_norm, cell_type=cell)


@pytest.mark.parametrize("batch_norm", [True, False], ids=["bn", "nobn"])
@pytest.mark.parametrize("activation", ["dice", "prelu"])
@pytest.mark.parametrize("cell", CELLS)
def test_model_forward_matches_restatement(cell, activation, batch_norm):
    m, inp = model_and_inputs(cell, activation, batch_norm)
    want = ref_forward(m, inp, cell, activation, batch_norm)
    m = m.cuda()
    with torch.no_grad():
        prob, logit, att = call(m, H.to_device(inp, "cuda"), return_attention=True)
        two = call(m, H.to_device(inp, "cuda"))
    torch.cuda.synchronize()
    report(f"logit {cell} {activation} bn={batch_norm}", logit, want[1])
    assert prob.shape == (64, 1) and logit.shape == (64, 1) and len(two) == 2
    torch.testing.assert_close(prob.double().cpu(), want[0], atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(logit.double().cpu(), want[1], atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(att.double().cpu(), want[2], **OP_TOL)
    assert torch.equal(two[0], prob) and torch.equal(two[1], logit)
    assert rankops.error_flags() == 0


def test_model_empty_batch_and_single_row():
    m, inp = model_and_inputs(B=1, T=50)
    want = ref_forward(m, inp, "AGRU", "dice", True)
    m = m.cuda()
    with torch.no_grad():
        prob, logit = call(m, H.to_device(inp, "cuda"))
        none = H.to_device(H.din_inputs(0, 50, H.SMALL_VOCAB), "cuda")
        p0, l0 = call(m, none)
    assert p0.shape == (0, 1) and l0.shape == (0, 1) and p0.dtype == torch.float32
    torch.testing.assert_close(logit.double().cpu(), want[1], atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(prob.double().cpu(), want[0], atol=1e-4, rtol=1e-4)


def test_model_wide_embedding_and_sixteen_units():
    torch.manual_seed(5)
    m = rankops.DIEN(None, hidden_units=[64, 32], custom_gru_type="AUGRU", gru_output_units=16,
                     vocab_sizes=H.SMALL_VOCAB, embedding_dim=32)
    H.randomize_eval_stats(m, 6)
    m.eval()
    inp = H.din_inputs(37, 20, H.SMALL_VOCAB, seed=7, min_len=0)
    want = dien_ref.forward(H.cpu_params(m), inp["dense"], inp["category"], inp["sequence"], inp["target"],
                            num_hidden=2, cell_type="AUGRU")
    m = m.cuda()
    with torch.no_grad():
        prob, logit = call(m, H.to_device(inp, "cuda"))
    torch.testing.assert_close(logit.double().cpu(), want[1], atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(prob.double().cpu(), want[0], atol=1e-4, rtol=1e-4)


def test_model_refuses_cpu_inputs_and_train_mode_on_the_gpu():
    m, inp = model_and_inputs(B=4, T=8)
    m = m.cuda()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        call(m, inp)
    with pytest.raises(NotImplementedError):
        call(m.train(), H.to_device(inp, "cuda"))


def test_model_forward_in_a_captured_graph_follows_its_inputs():
    m, first = model_and_inputs("AUGRU", B=64, T=50, seed=42)
    _, second = model_and_inputs("AUGRU", B=64, T=50, seed=91)
    m = m.cuda()
    static = H.to_device(first, "cuda")
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                call(m, static)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = call(m, static)
        g.replay()
        torch.cuda.synchronize()
        eager_first = call(m, H.to_device(first, "cuda"))
        assert torch.equal(out[0], eager_first[0]) and torch.equal(out[1], eager_first[1])

        def overwrite(dst, src):
            for k, v in src.items():
                if isinstance(v, dict):
                    overwrite(dst[k], v)
                else:
                    dst[k].copy_(v)
        overwrite(static, second)
        g.replay()
        torch.cuda.synchronize()
        eager_second = call(m, H.to_device(second, "cuda"))
    assert torch.equal(out[0], eager_second[0]) and torch.equal(out[1], eager_second[1])
    assert not torch.equal(eager_first[1], eager_second[1])
    assert rankops.error_flags() == 0
