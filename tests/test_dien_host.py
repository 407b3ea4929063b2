"""CPU tests of rankops.DIEN's host side (parameters, initialisation, refusals) and of the float64
restatement tests/dien_ref.py that the GPU tests compare against."""
import math

import pytest
import torch

import dien_ref
import helpers as H
import rankops


def build(seed=0, **kw):
    torch.manual_seed(seed)
    return rankops.DIEN(None, vocab_sizes=H.SMALL_VOCAB, **kw)


def inputs(B=4, T=6):
    return H.din_inputs(B, T, H.SMALL_VOCAB)


def test_state_dict_keys_and_shapes():
    m = build(hidden_units=[32, 16], gru_output_units=8)
    V = {f: n + 1 for f, n in H.SMALL_VOCAB.items()}
    rows = {k: v.shape[0] for k, v in m.state_dict().items() if k.startswith("embeddings.")}
    assert set(rows) == {f"embeddings.{f}.weight" for f in V}  # one feedid table: no history table
    got = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("embeddings.")}
    width = 16 + (16 + 2 + 4 + 4 + 4 + 4) + 16 + 8
    want = {
        "gru.gates.weight": (16, 24), "gru.gates.bias": (16,),
        "gru.candidate.weight": (8, 24), "gru.candidate.bias": (8,),
        "attention_project_matrix": (8, 16),
        "evolution.gates.weight": (16, 16), "evolution.gates.bias": (16,),
        "evolution.candidate.weight": (8, 16), "evolution.candidate.bias": (8,),
        "fcn.0.weight": (32, width), "fcn.0.bias": (32,),
        "fcn.1.alpha": (32,), "fcn.1.bn.running_mean": (32,), "fcn.1.bn.running_var": (32,),
        "fcn.1.bn.num_batches_tracked": (),
        "fcn.2.weight": (32,), "fcn.2.bias": (32,), "fcn.2.running_mean": (32,), "fcn.2.running_var": (32,),
        "fcn.2.num_batches_tracked": (),
        "fcn.4.weight": (16, 32), "fcn.4.bias": (16,),
        "fcn.5.alpha": (16,), "fcn.5.bn.running_mean": (16,), "fcn.5.bn.running_var": (16,),
        "fcn.5.bn.num_batches_tracked": (),
        "fcn.6.weight": (16,), "fcn.6.bias": (16,), "fcn.6.running_mean": (16,), "fcn.6.running_var": (16,),
        "fcn.6.num_batches_tracked": (),
        "output_layer.weight": (1, 16), "output_layer.bias": (1,),
    }
    assert got == want
    emb = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("embeddings.")}
    assert emb["embeddings.feedid.weight"][1] == 16 and emb["embeddings.userid.weight"][1] == 16
    assert [emb[f"embeddings.{f}.weight"][1] for f in ("device", "authorid", "bgm_song_id", "bgm_singer_id",
                                                       "manual_tag_list")] == [2, 4, 4, 4, 4]


def test_wide_embedding_and_units_shapes():
    m = build(hidden_units=[8], gru_output_units=16, embedding_dim=32, batch_norm=False, activation="prelu",
              dropout_rate=0.0)
    sd = m.state_dict()
    assert tuple(sd["gru.gates.weight"].shape) == (32, 48)
    assert tuple(sd["attention_project_matrix"].shape) == (16, 32)
    assert tuple(sd["evolution.candidate.weight"].shape) == (16, 32)
    assert tuple(sd["fcn.0.weight"].shape) == (8, 16 + 34 + 32 + 16)
    assert tuple(sd["fcn.1.weight"].shape) == (1,)  # PReLU
    assert "fcn.2.weight" not in sd


def test_initialisation_gate_biases_one_candidate_zero():
    m = build()
    for cell in (m.gru, m.evolution):
        assert torch.equal(cell["gates"].bias, torch.ones_like(cell["gates"].bias))
        assert torch.equal(cell["candidate"].bias, torch.zeros_like(cell["candidate"].bias))
        for lin in (cell["gates"], cell["candidate"]):  # Glorot uniform: |w| <= sqrt(6 / (fan_in + fan_out))
            bound = math.sqrt(6.0 / (lin.in_features + lin.out_features))
            assert lin.weight.abs().max() <= bound and lin.weight.abs().max() > 0.5 * bound
    bound = math.sqrt(6.0 / (8 + 16))
    assert m.attention_project_matrix.abs().max() <= bound


def test_seeded_construction_is_reproducible():
    a, b, c = build(3).state_dict(), build(3).state_dict(), build(4).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["gru.gates.weight"], c["gru.gates.weight"])


def test_cpu_forward_is_refused():
    m = build(hidden_units=[8]).eval()
    inp = inputs()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m(inp["dense"], inp["category"], inp["sequence"], inp["target"])
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        rankops.dien_interest(torch.zeros(2, 16), torch.zeros(2, 3, 16), torch.tensor([1, 2]),
                              dien_ref.draw_weights(16, 8, 0))


def test_train_mode_forward_is_not_implemented():
    m = build(hidden_units=[8]).train()
    inp = inputs()
    with pytest.raises(NotImplementedError):
        m(inp["dense"], inp["category"], inp["sequence"], inp["target"])


def test_unknown_gru_type_is_a_value_error():
    with pytest.raises(ValueError, match="AUGRU"):
        build(custom_gru_type="GRU")
    for ok in ("AGRU", "AUGRU"):
        assert build(custom_gru_type=ok).custom_gru_type == ok


# ------------------------------------------------------------------ the restatement itself

def _case(B=9, T=7, Hd=16, nh=8, seed=5):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Hd, generator=g)
    k = torch.randn(B, T, Hd, generator=g)
    lens = torch.randint(0, T + 1, (B,), generator=g)
    lens[:3] = torch.tensor([0, 1, T])
    return q, k, lens, dien_ref.draw_weights(Hd, nh, seed)


@pytest.mark.parametrize("cell", ["AGRU", "AUGRU"])
def test_restatement_ignores_keys_past_the_length(cell):
    q, k, lens, w = _case()
    s0, a0, _ = dien_ref.interest(q, k, lens, w, cell)
    k2 = k.clone()
    k2[torch.arange(k.shape[1])[None, :] >= lens[:, None]] = 1e3
    s1, a1, _ = dien_ref.interest(q, k2, lens, w, cell)
    assert torch.equal(s0, s1)
    valid = lens > 0  # with len = 0 the attention is uniform whatever the keys are
    assert torch.equal(a0[valid], a1[valid])
    assert torch.allclose(a0[~valid], torch.full_like(a0[~valid], 1.0 / k.shape[1]))
    assert torch.allclose(a1[~valid], torch.full_like(a1[~valid], 1.0 / k.shape[1]))


def test_restatement_ignores_ids_past_the_length():
    m = build(hidden_units=[8]).eval()
    H.randomize_eval_stats(m, 1)
    inp = inputs(B=8, T=6)
    p = H.cpu_params(m)
    out0 = dien_ref.forward(p, inp["dense"], inp["category"], inp["sequence"], inp["target"], num_hidden=1)
    seq = dict(inp["sequence"])
    ids, lens = seq[dien_ref.SEQ_KEY].clone(), seq[dien_ref.SEQ_KEY + "_length"]
    ids[torch.arange(ids.shape[1])[None, :] >= lens[:, None]] = H.SMALL_VOCAB["feedid"]  # the last row
    seq[dien_ref.SEQ_KEY] = ids
    out1 = dien_ref.forward(p, inp["dense"], inp["category"], seq, inp["target"], num_hidden=1)
    assert torch.equal(out0[0], out1[0]) and torch.equal(out0[1], out1[1])
    assert out0[0].shape == (8, 1) and out0[0].dtype == torch.float64


def test_restatement_zero_length_gives_zero_state():
    q, k, lens, w = _case()
    for cell in ("AGRU", "AUGRU"):
        s, a, _ = dien_ref.interest(q, k, lens, w, cell)
        assert torch.equal(s[0], torch.zeros(8, dtype=torch.float64))
        assert s[1:3].abs().min() > 0
        assert torch.allclose(a.sum(1), torch.ones(9, dtype=torch.float64))
        assert a[2].min() > 0 and torch.equal(a[1, 1:], torch.zeros(6, dtype=torch.float64))


def test_restatement_cells_differ():
    q, k, lens, w = _case()
    s0, a0, h0 = dien_ref.interest(q, k, lens, w, "AGRU")
    s1, a1, h1 = dien_ref.interest(q, k, lens, w, "AUGRU")
    assert torch.equal(a0, a1) and torch.equal(h0, h1)
    assert (s0 - s1)[lens > 1].abs().max() > 1e-2
    with pytest.raises(ValueError):
        dien_ref.interest(q, k, lens, w, "GRU")


def test_restatement_matches_hand_computation():
    """T = 1, H = nh = 1: every matrix is a number."""
    sig = lambda z: 1.0 / (1.0 + math.exp(-z))
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)
    x, q = 0.7, -1.3
    Wg, bg, Wc, bc, A = [[0.3, -0.2], [0.5, 0.4]], [1.1, 0.9], [[-0.6, 0.8]], [0.05], [[0.9]]
    Vg, vg, Vc, vc = [[0.2, 0.1], [-0.3, 0.25]], [1.2, 0.8], [[0.7, -0.4]], [-0.1]
    w = [f64(v) for v in (Wg, bg, Wc, bc, A, Vg, vg, Vc, vc)]
    # step 0 of the GRU from h = 0: r is multiplied by a zero state
    u = sig(0.5 * x + 0.9)
    c = math.tanh(-0.6 * x + 0.05)
    h0 = (1 - u) * c
    # one position: its attention weight is 1
    u2 = sig(-0.3 * h0 + 0.8)
    c2 = math.tanh(0.7 * h0 - 0.1)
    for cell, want in (("AGRU", c2), ("AUGRU", c2)):  # a = 1: AGRU takes c, AUGRU's u' = (1-a) u = 0
        s, a, hs = dien_ref.interest(f64([[q]]), f64([[[x]]]), torch.tensor([1]), w, cell)
        assert abs(hs.item() - h0) < 1e-14
        assert a.item() == 1.0
        assert abs(s.item() - want) < 1e-14
    # two positions, both valid: a second step exercises r*h, u*h and the softmax
    x1 = -0.4
    r = sig(0.3 * x1 - 0.2 * h0 + 1.1)
    u = sig(0.5 * x1 + 0.4 * h0 + 0.9)
    c = math.tanh(-0.6 * x1 + 0.8 * r * h0 + 0.05)
    h1 = u * h0 + (1 - u) * c
    e0, e1 = math.exp(h0 * 0.9 * q), math.exp(h1 * 0.9 * q)
    a0, a1 = e0 / (e0 + e1), e1 / (e0 + e1)
    s0_agru = a0 * c2
    s0_augru = (1 - (1 - a0) * u2) * c2
    for cell, s0 in (("AGRU", s0_agru), ("AUGRU", s0_augru)):
        r2 = sig(0.2 * h1 + 0.1 * s0 + 1.2)
        u3 = sig(-0.3 * h1 + 0.25 * s0 + 0.8)
        c3 = math.tanh(0.7 * h1 - 0.4 * r2 * s0 - 0.1)
        if cell == "AGRU":
            want = (1 - a1) * s0 + a1 * c3
        else:
            u3 = (1 - a1) * u3
            want = u3 * s0 + (1 - u3) * c3
        s, a, hs = dien_ref.interest(f64([[q]]), f64([[[x], [x1]]]), torch.tensor([2]), w, cell)
        assert abs(hs[0, 1].item() - h1) < 1e-14
        assert abs(a[0, 0].item() - a0) < 1e-14 and abs(a[0, 1].item() - a1) < 1e-14
        assert abs(s.item() - want) < 1e-14


def test_c_entry_points_validate_before_any_launch():
    """No device work is started on invalid input: these return on a machine without a GPU."""
    from rankops import _lib
    lib = _lib.load()
    one = 16  # any non-null address: validation never dereferences it
    w = [one] * 9
    assert lib.rk_dien_interest(None, 16, one, 10, 16, one, 5, 5, one, 2, 16, 8, 0, *w, one, 8, None, 0, None) == 1
    assert "rk_dien_interest" in _lib.last_error()
    assert lib.rk_dien_interest(one, 16, one, 10, 16, None, 5, 5, one, 2, 16, 8, 0, *w, one, 8, None, 0, None) == 1
    assert lib.rk_dien_interest(one, 16, one, 10, 16, one, 5, 0, one, 2, 16, 8, 0, *w, one, 8, None, 0, None) == 1
    assert lib.rk_dien_interest(one, 16, one, 10, 16, one, 5, 5, one, 2, 16, 8, 2, *w, one, 8, None, 0, None) == 1
    assert lib.rk_dien_interest(one, 16, one, 10, 16, one, 5, 5, one, 2, 16, 8, 0, *w, one, 4, None, 0, None) == 1
    assert lib.rk_dien_interest_dense(one, 16, None, 80, 16, 5, one, 2, 16, 8, 0, *w, one, 8, None, 0, None) == 1
    assert lib.rk_dien_interest_dense(one, 16, one, 80, 16, 5, one, 2, 16, 8, 0, *w, one, 8, one, 4, None) == 1
    for H_, nh, T in ((12, 8, 5), (16, 4, 5), (16, 8, 257), (64, 8, 5)):
        assert lib.rk_dien_interest(one, H_, one, 10, H_, one, T, T, one, 2, H_, nh, 0, *w, one, nh, None, 0,
                                    None) == 4
        assert lib.rk_dien_interest_dense(one, H_, one, T * H_, H_, T, one, 2, H_, nh, 1, *w, one, nh, None, 0,
                                          None) == 4
        assert "envelope" in _lib.last_error()
    # an empty batch is a valid call that launches nothing
    assert lib.rk_dien_interest(one, 16, one, 10, 16, one, 5, 5, one, 0, 16, 8, 0, *w, one, 8, None, 0, None) == 0
