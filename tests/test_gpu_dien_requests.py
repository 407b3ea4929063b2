"""GPU tests of request-level DIEN scoring: rk_dien_extract(_dense) / rk_dien_evolve through
rankops.dien_extract(_gather) / dien_evolve, and DIEN.extract_interests / score.

The main checks need no tolerance: the two kernels call the fused kernel's code on the same values,
so extract's hs is torch.equal to the train forward's and evolve's state and attention are
torch.equal to rk_dien_interest on the history replicated per candidate.  Against the float64
restatement tests/dien_ref.py the bound is the project's op bound, atol 1e-5, rtol 0, which
tests/test_dien_requests_ref.py keeps at ten times or more above the fp32 drift of the restatement
on these very draws (tests/dien_requests_cases.py).  Model outputs use the project's 1e-4 / 1e-4."""
import functools

import pytest
import torch

import dien_ref
import dien_requests_cases as C
import helpers as H
import rankops
from rankops import _lib, ops

pytestmark = pytest.mark.gpu

CELLS, CASES, OP_TOL, VOCAB = C.CELLS, C.CASES, C.OP_TOL, C.VOCAB
BIG = (5, 67, 50, 16, 8)
cases = pytest.mark.parametrize("c", CASES, ids=C.case_id)
cells = pytest.mark.parametrize("cell", CELLS)


def cuda(*ts):
    return [t.cuda() if isinstance(t, torch.Tensor) else [x.cuda() for x in t] for t in ts]


def report(name, got, want):
    err = (got.double().cpu() - want).abs().max().item() if want.numel() else 0.0
    print(f"{name}: max |err| = {err:.3e}")


def past_the_length(lens, T):
    return torch.arange(T)[None, :] >= lens[:, None]


@functools.lru_cache(maxsize=None)
def split(c, cell):
    """(hs, state, attention) of extract + evolve on the case, on the GPU; never modified."""
    q, table, ids, lens, req, w = cuda(*C.case(*c))
    hs = rankops.dien_extract_gather(table, ids, lens, w)
    s, a = rankops.dien_evolve(q, hs, lens, req, w, cell, return_attention=True)
    return hs, s, a


@cases
def test_extract_is_bit_equal_to_the_train_forward_states(c):
    R, B, T, Hd, nh = c
    q, table, ids, lens, req, w = C.case(*c)
    dt, di, dl, dw = cuda(table, ids, lens, w)
    hs = rankops.dien_extract_gather(dt, di, dl, dw)
    torch.cuda.synchronize()
    assert hs.shape == (R, T, nh) and hs.dtype == torch.float32 and hs.grad_fn is None and not hs.requires_grad
    any_query = torch.full((R, Hd), 0.37, device="cuda")  # hs does not depend on it
    for cell in CELLS:
        _, want = rankops.dien_interest_gather(any_query, dt, di, dl, dw, cell, return_states=True)
        assert torch.equal(hs, want), cell
    assert torch.equal(hs.cpu()[past_the_length(lens, T)], torch.zeros(int(past_the_length(lens, T).sum()), nh))
    assert torch.equal(rankops.dien_extract(dt[di], dl, dw), hs)  # the dense form
    ref = C.reference(*c, "AGRU")[2]
    report(f"hs {c}", hs, ref)
    torch.testing.assert_close(hs.double().cpu(), ref, **OP_TOL)
    assert rankops.error_flags() == 0


@cells
@cases
def test_evolve_is_bit_equal_to_the_fused_kernel_on_replicated_histories(c, cell):
    R, B, T, Hd, nh = c
    q, table, ids, lens, req, w = C.case(*c)
    dq, dt, di, dl, dr, dw = cuda(q, table, ids, lens, req, w)
    hs, s, a = split(c, cell)
    torch.cuda.synchronize()
    assert s.shape == (B, nh) and a.shape == (B, T) and s.dtype == torch.float32 and s.grad_fn is None
    want_s, want_a = rankops.dien_interest_gather(dq, dt, di[dr], dl[dr], dw, cell, return_attention=True)
    assert torch.equal(s, want_s)
    assert torch.equal(a, want_a)
    ref_s, ref_a, _ = C.reference(*c, cell)
    report(f"state {c} {cell}", s, ref_s)
    report(f"attention {c} {cell}", a, ref_a)
    torch.testing.assert_close(s.double().cpu(), ref_s, **OP_TOL)
    torch.testing.assert_close(a.double().cpu(), ref_a, **OP_TOL)
    empty = lens[req] == 0
    assert torch.equal(s.cpu()[empty], torch.zeros(int(empty.sum()), nh))
    assert torch.equal(rankops.dien_evolve(dq, hs, dl, dr, dw, cell), s)  # without the attention output
    assert rankops.error_flags() == 0


@cells
def test_poisoned_inputs_past_the_length_change_nothing(cell):
    R, B, T, Hd, nh = BIG
    q, table, ids, lens, req, w = C.case(*BIG)
    dq, dt, dl, dr, dw = cuda(q, table, lens, req, w)
    hs, s, a = split(BIG, cell)
    past = past_the_length(lens, T)
    for poison in (VOCAB - 1, VOCAB + 5, -1, 2 ** 40):  # ids at t >= len are never read
        bad = ids.clone()
        bad[past] = poison
        assert torch.equal(rankops.dien_extract_gather(dt, bad.cuda(), dl, dw), hs), poison
        assert rankops.error_flags() == 0, poison
    bad_hs = hs.clone()  # rows of hs at t >= len are never read
    bad_hs[past.cuda()] = float("nan")
    got = rankops.dien_evolve(dq, bad_hs, dl, dr, dw, cell, return_attention=True)
    assert torch.equal(got[0], s) and torch.equal(got[1], a)
    assert rankops.error_flags() == 0


def test_out_of_range_history_id_reads_a_zero_row_and_raises_the_flag():
    R, B, T, Hd, nh = BIG
    q, table, ids, lens, req, w = C.case(*BIG)
    r = next(int(x) for x in torch.nonzero(lens >= 5).flatten() if int(x) in set(req.tolist()))
    bad = ids.clone()
    bad[r, 3] = VOCAB  # one past the last row, at t = 3 < len
    keys = table[ids].clone()
    keys[r, 3] = 0.0
    want_s, want_a, _ = dien_ref.interest(q, keys[req], lens[req], w, "AUGRU")
    _, _, want_hs = dien_ref.interest(q[:R], keys, lens, w, "AUGRU")
    want_hs = want_hs * (~past_the_length(lens, T))[:, :, None]
    dq, dt, dl, dr, dw = cuda(q, table, lens, req, w)
    assert rankops.error_flags() == 0
    hs = rankops.dien_extract_gather(dt, bad.cuda(), dl, dw)
    flags = rankops.error_flags()  # reads and resets
    assert flags & _lib.RK_FLAG_INDEX_OOB
    assert rankops.error_flags() == 0
    s, a = rankops.dien_evolve(dq, hs, dl, dr, dw, "AUGRU", return_attention=True)
    torch.testing.assert_close(hs.double().cpu(), want_hs, **OP_TOL)
    torch.testing.assert_close(s.double().cpu(), want_s, **OP_TOL)
    torch.testing.assert_close(a.double().cpu(), want_a, **OP_TOL)
    clean = C.reference(*BIG, "AUGRU")[0]
    assert (want_s - clean)[req == r].abs().max() > 1e-4  # the zero row does change this request's candidates
    assert rankops.error_flags() == 0


@cells
def test_out_of_range_request_index_gives_a_zero_state_and_raises_the_flag(cell):
    R, B, T, Hd, nh = BIG
    q, table, ids, lens, req, w = C.case(*BIG)
    hs, s, a = split(BIG, cell)
    bad = req.clone()
    below, above = 5, B - 2  # one in a full wave, one in the partly filled last wave
    bad[below], bad[above] = -1, R
    dq, dl, dw = cuda(q, lens, w)
    assert rankops.error_flags() == 0
    got_s, got_a = rankops.dien_evolve(dq, hs, dl, bad.cuda(), dw, cell, return_attention=True)
    assert rankops.error_flags() & _lib.RK_FLAG_INDEX_OOB
    assert rankops.error_flags() == 0
    keep = torch.ones(B, dtype=torch.bool)
    keep[[below, above]] = False
    assert torch.equal(got_s[keep.cuda()], s[keep.cuda()]) and torch.equal(got_a[keep.cuda()], a[keep.cuda()])
    assert torch.equal(got_s[~keep.cuda()], torch.zeros(2, nh, device="cuda"))
    empty = int(torch.nonzero(lens[req] == 0)[0])  # a candidate of the request with an empty history
    assert torch.equal(got_a[below], a[empty]) and torch.equal(got_a[above], a[empty])
    torch.testing.assert_close(got_a[below].cpu(), torch.full((T,), 1.0 / T), atol=1e-7, rtol=0)


@cells
def test_strided_query_and_output_in_one_row(cell):
    R, B, T, Hd, nh = BIG
    q, table, ids, lens, req, w = C.case(*BIG)
    dl, dr, dw = cuda(lens, req, w)
    hs, s, _ = split(BIG, cell)
    width, q_col = 3 + Hd + 5 + nh, 3  # [3 | query | 5 | state]: the query is not 16-B aligned
    row = torch.full((B, width), 777.0, device="cuda")
    row[:, q_col:q_col + Hd] = q.cuda()
    before = row.clone()
    ops.dien_evolve(_lib.fptr(row, q_col), width, hs, dl, dr, Hd, ops.DIEN_CELLS[cell], dw[4:],
                    _lib.fptr(row, width - nh), width, None, B, row.device)
    torch.cuda.synchronize()
    assert torch.equal(row[:, :width - nh], before[:, :width - nh])
    assert torch.equal(row[:, width - nh:], s)
    torch.testing.assert_close(row[:, width - nh:].double().cpu(), C.reference(*BIG, cell)[0], **OP_TOL)


@pytest.mark.parametrize("c", [BIG, (2, 9, 200, 32, 16)], ids=C.case_id)
def test_two_launches_are_bit_equal(c):
    q, table, ids, lens, req, w = cuda(*C.case(*c))
    for cell in CELLS:
        hs, s, a = split(c, cell)
        hs2 = rankops.dien_extract_gather(table, ids, lens, w)
        s2, a2 = rankops.dien_evolve(q, hs2, lens, req, w, cell, return_attention=True)
        assert torch.equal(hs, hs2) and torch.equal(s, s2) and torch.equal(a, a2)


def test_extract_and_evolve_in_a_captured_graph_follow_their_inputs():
    first, second = C.case(*BIG), C.case(*BIG, seed=23)
    q, table, ids, lens, req, w = cuda(*first)
    q, ids, lens, req = q.clone(), ids.clone(), lens.clone(), req.clone()  # the graph's static inputs

    def run():
        hs = rankops.dien_extract_gather(table, ids, lens, w)
        return (hs,) + rankops.dien_evolve(q, hs, lens, req, w, "AUGRU", return_attention=True)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run()
    g.replay()
    torch.cuda.synchronize()
    eager_first = [t.clone() for t in run()]
    assert all(torch.equal(o, e) for o, e in zip(out, eager_first))
    for dst, src in zip((q, ids, lens, req), (second[0], second[2], second[3], second[4])):
        dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    eager_second = run()
    assert all(torch.equal(o, e) for o, e in zip(out, eager_second))
    assert not torch.equal(eager_first[1], eager_second[1])
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("T,Hd,nh", [(3, 12, 8), (3, 16, 4), (257, 16, 8)])
def test_outside_the_envelope_is_not_implemented(T, Hd, nh):
    R, B = 2, 3
    g = torch.Generator().manual_seed(0)
    q, k = torch.randn(B, Hd, generator=g).cuda(), torch.randn(R, T, Hd, generator=g).cuda()
    lens, req = torch.full((R,), T).cuda(), torch.tensor([1, 0, 1]).cuda()
    w = [x.cuda() for x in dien_ref.draw_weights(Hd, nh, 0)]
    with pytest.raises(NotImplementedError, match="envelope"):
        rankops.dien_extract(k, lens, w)
    with pytest.raises(NotImplementedError, match="envelope"):
        rankops.dien_extract_gather(torch.randn(9, Hd, generator=g).cuda(),
                                    torch.zeros(R, T, dtype=torch.int64, device="cuda"), lens, w)
    hs = torch.zeros(R, T, nh, device="cuda")
    with pytest.raises(NotImplementedError, match="envelope"):
        rankops.dien_evolve(q, hs, lens, req, w)
    with pytest.raises(rankops.RankOpsError) as e:  # the C entry points themselves refuse, before any launch
        ops.dien_extract_dense(k, lens, nh, w[:4], hs)
    assert e.value.code == _lib.RK_ERR_UNSUPPORTED
    out = torch.empty(B, nh, device="cuda")
    with pytest.raises(rankops.RankOpsError) as e:
        ops.dien_evolve(q.data_ptr(), Hd, hs, lens, req, Hd, 0, w[4:], out.data_ptr(), nh, None, B, q.device)
    assert e.value.code == _lib.RK_ERR_UNSUPPORTED


def test_bad_arguments_are_value_errors_and_cpu_tensors_raise():
    c = (3, 7, 3, 8, 8)
    q, table, ids, lens, req, w = C.case(*c)
    dq, dt, di, dl, dr, dw = cuda(q, table, ids, lens, req, w)
    hs = rankops.dien_extract_gather(dt, di, dl, dw)
    with pytest.raises(ValueError):
        rankops.dien_extract_gather(dt, di, dl[:2], dw)
    with pytest.raises(ValueError):
        rankops.dien_extract_gather(dt, di, dl, dw[:8])
    with pytest.raises(ValueError):
        rankops.dien_extract(dt[di], dl[:2], dw)
    with pytest.raises(ValueError):
        rankops.dien_extract(dt[di][0], dl, dw)
    with pytest.raises(ValueError):
        rankops.dien_evolve(dq, hs, dl, dr, dw, "GRU")
    with pytest.raises(ValueError):
        rankops.dien_evolve(dq, hs, dl, dr[:5], dw)  # one request per query row
    with pytest.raises(ValueError):
        rankops.dien_evolve(dq, hs, dl[:2], dr, dw)
    with pytest.raises(ValueError):
        rankops.dien_evolve(dq[:, :4], hs, dl, dr, dw)
    with pytest.raises(ValueError):
        rankops.dien_evolve(dq, hs[:, :, :4], dl, dr, dw)
    with pytest.raises(ValueError):
        rankops.dien_evolve(dq, hs[:0], dl[:0], dr, dw)  # candidates, but no request to name
    for args in ((q, hs, dl, dr, dw), (dq, hs.cpu(), dl, dr, dw), (dq, hs, lens, dr, dw), (dq, hs, dl, req, dw)):
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            rankops.dien_evolve(*args)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rankops.dien_extract_gather(table, di, dl, dw)
    s0, a0 = rankops.dien_evolve(dq[:0], hs, dl, dr[:0], dw, return_attention=True)  # no candidate
    assert s0.shape == (0, 8) and a0.shape == (0, 3)
    assert rankops.dien_extract_gather(dt, di[:0], dl[:0], dw).shape == (0, 3, 8)  # no request
    assert rankops.error_flags() == 0


# ------------------------------------------------------------------ the module

SEQ, SEQ_LEN = dien_ref.SEQ_KEY, dien_ref.SEQ_KEY + "_length"


def model_and_requests(cell="AGRU", activation="dice", batch_norm=True, R=5, B=64, T=50, seed=42):
    """An eval model, the R requests' histories, B candidates (forward's inputs with each request's
    history repeated for its candidates) and their request_index."""
    torch.manual_seed(seed)
    m = rankops.DIEN(None, activation=activation, batch_norm=batch_norm, custom_gru_type=cell,
                     vocab_sizes=H.SMALL_VOCAB)
    H.randomize_eval_stats(m, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():  # gate biases away from 1, candidate biases away from 0
        for cellm in (m.gru, m.evolution):
            for lin in cellm.values():
                lin.bias.add_(0.5 * (torch.rand(lin.bias.shape, generator=g) - 0.5))
    history = H.din_inputs(R, T, H.SMALL_VOCAB, seed=seed + 4)["sequence"]
    if R >= 3:
        history[SEQ_LEN][:3] = torch.tensor([0, 1, T])
    inp = H.din_inputs(B, T, H.SMALL_VOCAB, seed=seed + 3)
    req = torch.randint(0, R, (B,), generator=g)
    inp["sequence"] = {SEQ: history[SEQ][req], SEQ_LEN: history[SEQ_LEN][req]}
    return m.eval(), history, inp, req


def forward(m, inp, **kw):
    return m(inp["dense"], inp["category"], inp["sequence"], inp["target"], **kw)


def score(m, inp, interests, req, **kw):
    return m.score(inp["dense"], inp["category"], inp["target"], interests, req, **kw)


@pytest.mark.parametrize("batch_norm", [True, False], ids=["bn", "nobn"])
@pytest.mark.parametrize("activation", ["dice", "prelu"])
@cells
def test_model_score_is_bit_equal_to_forward_on_replicated_histories(cell, activation, batch_norm):
    m, history, inp, req = model_and_requests(cell, activation, batch_norm)
    want = dien_ref.forward(H.cpu_params(m), inp["dense"], inp["category"], inp["sequence"], inp["target"],
                            activation=activation, batch_norm=batch_norm, cell_type=cell)
    m = m.cuda()
    d_inp, d_hist, d_req = H.to_device(inp, "cuda"), H.to_device(history, "cuda"), req.cuda()
    with torch.no_grad():
        fused = forward(m, d_inp, return_attention=True)
    interests = m.extract_interests(d_hist)  # no torch.no_grad() needed: inference only
    prob, logit, att = score(m, d_inp, interests, d_req, return_attention=True)
    two = score(m, d_inp, interests, d_req)
    torch.cuda.synchronize()
    assert isinstance(interests, rankops.DIENInterests) and interests.hs.shape == (5, 50, 8) and len(interests) == 5
    assert prob.shape == (64, 1) and logit.shape == (64, 1) and len(two) == 2
    assert prob.grad_fn is None and logit.grad_fn is None and interests.hs.grad_fn is None
    assert torch.equal(prob, fused[0]) and torch.equal(logit, fused[1]) and torch.equal(att, fused[2])
    assert torch.equal(two[0], prob) and torch.equal(two[1], logit)
    report(f"logit {cell} {activation} bn={batch_norm}", logit, want[1])
    torch.testing.assert_close(prob.double().cpu(), want[0], atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(logit.double().cpu(), want[1], atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(att.double().cpu(), want[2], **OP_TOL)
    assert rankops.error_flags() == 0


def test_model_one_interests_object_scores_different_candidate_sets():
    m, history, inp, req = model_and_requests("AUGRU")
    _, _, other, other_req = model_and_requests("AUGRU", B=23, seed=77)
    other["sequence"] = {SEQ: history[SEQ][other_req], SEQ_LEN: history[SEQ_LEN][other_req]}
    m = m.cuda()
    d_hist = H.to_device(history, "cuda")
    cached = m.extract_interests(d_hist)
    kept = cached.hs.clone()
    for cand, r in ((inp, req), (other, other_req)):
        d = H.to_device(cand, "cuda")
        got = score(m, d, cached, r.cuda())
        fresh = score(m, d, m.extract_interests(d_hist), r.cuda())
        with torch.no_grad():
            fused = forward(m, d)
        assert torch.equal(got[0], fresh[0]) and torch.equal(got[1], fresh[1])
        assert torch.equal(got[0], fused[0]) and torch.equal(got[1], fused[1])
    assert torch.equal(cached.hs, kept)
    assert rankops.error_flags() == 0


def test_model_empty_candidate_batch_one_candidate_and_train_mode():
    m, history, inp, req = model_and_requests(B=1)
    want = dien_ref.forward(H.cpu_params(m), inp["dense"], inp["category"], inp["sequence"], inp["target"])
    m = m.cuda()
    d_inp, d_hist = H.to_device(inp, "cuda"), H.to_device(history, "cuda")
    interests = m.extract_interests(d_hist)
    prob, logit = score(m, d_inp, interests, req.cuda())
    torch.testing.assert_close(logit.double().cpu(), want[1], atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(prob.double().cpu(), want[0], atol=1e-4, rtol=1e-4)
    none = H.to_device(H.din_inputs(0, 50, H.SMALL_VOCAB), "cuda")
    p0, l0, a0 = score(m, none, interests, req.cuda()[:0], return_attention=True)
    assert p0.shape == (0, 1) and l0.shape == (0, 1) and a0.shape == (0, 50) and p0.dtype == torch.float32
    assert len(score(m, none, interests, req.cuda()[:0])) == 2
    with pytest.raises(ValueError):
        score(m, d_inp, interests, torch.tensor([0, 1]).cuda())  # two requests named for one candidate
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        score(m, inp, interests, req.cuda())
    m.train()
    with pytest.raises(NotImplementedError):
        m.extract_interests(d_hist)
    with pytest.raises(NotImplementedError):
        score(m, d_inp, interests, req.cuda())
    assert rankops.error_flags() == 0
