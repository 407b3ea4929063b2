"""CPU tests of request-level DIEN scoring (rk_dien_extract / rk_dien_evolve, rankops.dien_extract /
dien_evolve, DIEN.extract_interests / score): the tolerance of the GPU tests re-measured on their own
draws, the split restated, and the host side (exports, argument validation before any launch,
refusals)."""
import pytest
import torch

import dien_ref
import dien_requests_cases as C
import helpers as H
import rankops


def test_op_tolerance_is_at_least_ten_times_the_fp32_drift():
    """tests/test_gpu_dien_requests.py compares with the float64 restatement at atol 1e-5.  That
    bound means something only while it stays well above what fp32 arithmetic alone does to the
    restatement on the committed draws (3.2e-7 to 3.8e-7 at most when this was written, depending on
    the host's BLAS; worst at T 200, H 32, nh 16): fail if someone changes the draws so that 1e-5
    is less than ten times the drift."""
    worst = 0.0
    for c in C.CASES:
        for cell in C.CELLS:
            want = C.reference(*c, cell)
            got = C.reference(*c, cell, torch.float32)
            drift = max((g.double() - w).abs().max().item() for g, w in zip(got, want))
            print(f"{C.case_id(c)} {cell}: fp32 drift {drift:.3e}")
            worst = max(worst, drift)
    assert worst > 0.0
    assert C.OP_TOL["atol"] >= 10 * worst, worst
    assert C.OP_TOL["rtol"] == 0


def test_cases_are_what_the_gpu_tests_rely_on():
    for R, B, T, Hd, nh in C.CASES:
        q, table, ids, lens, req, w = C.case(R, B, T, Hd, nh)
        assert q.shape == (B, Hd) and ids.shape == (R, T) and lens.shape == (R,) and req.shape == (B,)
        assert lens.tolist()[:3] == {1: [T], 2: [1, T]}.get(R, [0, 1, T])
        assert 0 <= int(req.min()) and int(req.max()) < R
        if B > 1:
            assert not torch.equal(req, req.sort().values)  # unsorted
        if B >= R:
            want = set(range(R)) - ({C.UNUSED_REQUEST} if R == 5 else set())
            assert set(req.tolist()) == want
    assert any(B % 4 for _, B, _, _, _ in C.CASES)  # a partly filled last wave


@pytest.mark.parametrize("cell", C.CELLS)
def test_extractor_states_do_not_depend_on_the_query_or_the_cell(cell):
    """What makes the split exact: hs is a function of the history and the extractor weights."""
    c = (5, 67, 50, 16, 8)
    q, table, ids, lens, req, w = C.case(*c)
    _, _, hs0 = dien_ref.interest(torch.zeros(5, 16), table[ids], lens, w, cell)
    _, _, hs1 = dien_ref.interest(q[:5], table[ids], lens, w, "AGRU")
    assert torch.equal(hs0, hs1)
    _, _, per_candidate = dien_ref.interest(q, table[ids[req]], lens[req], w, cell)
    # a BLAS may sum a batch of 67 rows in another order than a batch of 5: float64 rounding, no more
    torch.testing.assert_close(per_candidate, hs0[req], atol=1e-13, rtol=0)


def test_new_names_are_exported():
    for name in ("dien_extract", "dien_extract_gather", "dien_evolve", "DIENInterests"):
        assert name in rankops.__all__ and callable(getattr(rankops, name))
    assert callable(rankops.DIEN.extract_interests) and callable(rankops.DIEN.score)
    for fn in (rankops.dien_extract, rankops.dien_extract_gather, rankops.dien_evolve):
        assert "Inference only" in fn.__doc__ and "dien_interest" in fn.__doc__
    assert "weight update" in rankops.DIEN.extract_interests.__doc__


def test_cpu_tensors_are_refused():
    w = dien_ref.draw_weights(16, 8, 0)
    lens, req = torch.tensor([1, 2]), torch.tensor([0, 1, 1])
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rankops.dien_extract(torch.zeros(2, 3, 16), lens, w)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rankops.dien_extract_gather(torch.zeros(9, 16), torch.zeros(2, 3, dtype=torch.int64), lens, w)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rankops.dien_evolve(torch.zeros(3, 16), torch.zeros(2, 3, 8), lens, req, w)
    m = rankops.DIEN(None, hidden_units=[8], vocab_sizes=H.SMALL_VOCAB).eval()
    inp = H.din_inputs(3, 6, H.SMALL_VOCAB)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.extract_interests(inp["sequence"])
    cached = rankops.DIENInterests(torch.zeros(2, 6, 8), lens)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.score(inp["dense"], inp["category"], inp["target"], cached, req)


def test_train_mode_is_refused():
    m = rankops.DIEN(None, hidden_units=[8], vocab_sizes=H.SMALL_VOCAB, trainable=True).train()
    inp = H.din_inputs(3, 6, H.SMALL_VOCAB)
    with pytest.raises(NotImplementedError, match="eval"):
        m.extract_interests(inp["sequence"])
    with pytest.raises(NotImplementedError, match="eval"):
        m.score(inp["dense"], inp["category"], inp["target"], rankops.DIENInterests(torch.zeros(2, 6, 8),
                                                                                    torch.tensor([1, 2])),
                torch.tensor([0, 1, 1]))


def test_c_entry_points_validate_before_any_launch():
    """No device work is started on invalid input: these return on a machine without a GPU."""
    from rankops import _lib
    lib = _lib.load()
    INVALID, UNSUPPORTED = 1, _lib.RK_ERR_UNSUPPORTED  # RK_ERR_INVALID, include/rankops.h
    one = 16  # any non-null, 16-B aligned address: validation never dereferences it
    w4, w5 = [one] * 4, [one] * 5
    # rk_dien_extract(key_table, key_rows, ld_key, seq, ld_seq, T, seq_len, requests, H, nh, Wg, bg, Wc, bc, hs, stream)
    ok = (one, 10, 16, one, 5, 5, one, 2, 16, 8, *w4, one, None)
    for i in (0, 3, 6, 10, 13, 14):  # null pointers
        bad = list(ok)
        bad[i] = None
        assert lib.rk_dien_extract(*bad) == INVALID, i
        assert "rk_dien_extract" in _lib.last_error()
    for i, v in ((1, 0), (2, 8), (4, 4), (5, 0), (7, -1)):  # key_rows, ld_key < H, ld_seq < T, T, requests
        bad = list(ok)
        bad[i] = v
        assert lib.rk_dien_extract(*bad) == INVALID, i
    assert lib.rk_dien_extract(one, 10, 18, one, 5, 5, one, 2, 16, 8, *w4, one, None) == UNSUPPORTED
    assert lib.rk_dien_extract(20, 10, 16, one, 5, 5, one, 2, 16, 8, *w4, one, None) == UNSUPPORTED
    assert "aligned" in _lib.last_error()
    assert lib.rk_dien_extract(one, 10, 16, one, 5, 5, one, 0, 16, 8, *w4, one, None) == 0  # no request, no launch
    # rk_dien_extract_dense(keys, ld_keys_b, ld_keys_t, T, keys_length, requests, H, nh, Wg, bg, Wc, bc, hs, stream)
    okd = (one, 80, 16, 5, one, 2, 16, 8, *w4, one, None)
    for i in (0, 4, 8, 12):
        bad = list(okd)
        bad[i] = None
        assert lib.rk_dien_extract_dense(*bad) == INVALID, i
    assert lib.rk_dien_extract_dense(one, 64, 16, 5, one, 2, 16, 8, *w4, one, None) == INVALID
    assert lib.rk_dien_extract_dense(one, 80, 16, 5, one, 0, 16, 8, *w4, one, None) == 0
    # rk_dien_evolve(query, ld_query, hs, requests, T, seq_len, request_index, batch, H, nh, cell, A, Vg, vg, Vc,
    #                vc, out, ld_out, att_out, ld_att, stream)
    oke = (one, 16, one, 2, 5, one, one, 3, 16, 8, 0, *w5, one, 8, None, 0, None)
    for i in (0, 2, 5, 6, 11, 15, 16):
        bad = list(oke)
        bad[i] = None
        assert lib.rk_dien_evolve(*bad) == INVALID, i
        assert "rk_dien_evolve" in _lib.last_error()
    for i, v in ((1, 8), (3, -1), (4, 0), (7, -1), (10, 2), (17, 4)):  # ld_query, requests, T, batch, cell, ld_out
        bad = list(oke)
        bad[i] = v
        assert lib.rk_dien_evolve(*bad) == INVALID, i
    bad = list(oke)
    bad[18], bad[19] = one, 4  # att_out with ld_att < T
    assert lib.rk_dien_evolve(*bad) == INVALID
    bad = list(oke)
    bad[2] = 24  # hs not 16-B aligned
    assert lib.rk_dien_evolve(*bad) == UNSUPPORTED
    for H_, nh, T in ((12, 8, 5), (16, 4, 5), (16, 8, 257), (64, 8, 5)):
        assert lib.rk_dien_extract(one, 10, H_, one, T, T, one, 2, H_, nh, *w4, one, None) == UNSUPPORTED
        assert lib.rk_dien_extract_dense(one, T * H_, H_, T, one, 2, H_, nh, *w4, one, None) == UNSUPPORTED
        assert lib.rk_dien_evolve(one, H_, one, 2, T, one, one, 3, H_, nh, 1, *w5, one, nh, None, 0,
                                  None) == UNSUPPORTED
        assert "envelope" in _lib.last_error()
    for batch, requests in ((0, 2), (3, 0), (0, 0)):  # valid calls that launch nothing
        assert lib.rk_dien_evolve(one, 16, one, requests, 5, one, one, batch, 16, 8, 0, *w5, one, 8, None, 0, None) == 0
