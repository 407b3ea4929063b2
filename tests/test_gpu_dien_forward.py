"""GPU tests of the one-launch DIEN eval forward (rk_dien_forward, csrc/dien_forward.hip) and of
DIEN.prepare.

The main check needs no tolerance: the kernel calls rk_dien_interest's phases on the same values and
runs the tail on the plan rk_mlp_forward picks, so prob, logit and the attention are torch.equal to
the three launches (rk_concat_gather, rk_dien_interest, the tail) of the same model, which the tests
get by switching rankops.common.FUSED_DIEN off.  Against the float64 restatement tests/dien_ref.py the
bound is the module's, atol = rtol = 1e-4 (tests/test_gpu_dien_requests.py).

Cases (B, T, H) at nh 8: (1, 1, 16) one live quarter of one chain wave; (7, 3, 8) a partly filled
second chain wave; (16, 50, 16) a full workgroup; (17, 50, 16) a second workgroup with one row;
(67, 50, 32) five workgroups at the widest row.  Lengths 0, 1 and T are forced into the first
samples (B 1: T; B 2: 1, T)."""
import functools

import pytest
import torch

import dien_ref
import helpers as H
import rankops
from rankops import _lib, common, ops

pytestmark = pytest.mark.gpu

CELLS = ("AGRU", "AUGRU")
CASES = [(1, 1, 16), (7, 3, 8), (16, 50, 16), (17, 50, 16), (67, 50, 32)]
SEQ, SEQ_LEN = dien_ref.SEQ_KEY, dien_ref.SEQ_KEY + "_length"
TOL = dict(atol=1e-4, rtol=1e-4)
cells = pytest.mark.parametrize("cell", CELLS)


def make(B, T, Hd, cell, activation="dice", batch_norm=True, nh=8, seed=42):
    """An eval model on the CPU and its inputs."""
    torch.manual_seed(seed)
    m = rankops.DIEN(None, activation=activation, batch_norm=batch_norm, custom_gru_type=cell, gru_output_units=nh,
                     vocab_sizes=H.SMALL_VOCAB, embedding_dim=Hd)
    H.randomize_eval_stats(m, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():  # gate biases away from 1, candidate biases away from 0
        for cellm in (m.gru, m.evolution):
            for lin in cellm.values():
                lin.bias.add_(0.5 * (torch.rand(lin.bias.shape, generator=g) - 0.5))
    inp = H.din_inputs(B, T, H.SMALL_VOCAB, seed=seed + 3)
    forced = {1: [T], 2: [1, T]}.get(B, [0, 1, T])
    inp["sequence"][SEQ_LEN][:len(forced)] = torch.tensor(forced)
    return m.eval(), inp


@functools.lru_cache(maxsize=None)
def setup(c, cell, activation="dice", batch_norm=True):
    """(model on the GPU, inputs on the CPU, inputs on the GPU, float64 reference); never modified."""
    m, inp = make(*c, cell, activation, batch_norm)
    want = dien_ref.forward(H.cpu_params(m), inp["dense"], inp["category"], inp["sequence"], inp["target"],
                            activation=activation, batch_norm=batch_norm, cell_type=cell)
    return m.cuda(), inp, H.to_device(inp, "cuda"), want


def forward(m, d, fused, monkeypatch, **kw):
    """The eval forward with the one launch switched on or off (off: the three launches)."""
    with monkeypatch.context() as mp:
        mp.setattr(common, "FUSED_DIEN", fused)
        with torch.no_grad():
            out = m(d["dense"], d["category"], d["sequence"], d["target"], **kw)
    torch.cuda.synchronize()
    return out


def refuse(name):
    def f(*a, **k):
        raise AssertionError(f"{name} was called")
    return f


def only_the_fused_launch(mp):
    mp.setattr(ops, "concat_gather", refuse("ops.concat_gather"))
    mp.setattr(ops, "dien_interest", refuse("ops.dien_interest"))
    mp.setattr(rankops.dien, "run_tail", refuse("run_tail"))


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def check(c, cell, activation, batch_norm, monkeypatch):
    B, T, Hd = c
    m, inp, d, want = setup(c, cell, activation, batch_norm)
    assert rankops.error_flags() == 0
    fused = forward(m, d, True, monkeypatch, return_attention=True)
    assert not m.__dict__.get("_unfusable")  # it was the one launch that answered
    three = forward(m, d, False, monkeypatch, return_attention=True)
    prob, logit, att = fused
    assert prob.shape == (B, 1) and logit.shape == (B, 1) and att.shape == (B, T) and prob.dtype == torch.float32
    assert torch.equal(prob, three[0]) and torch.equal(logit, three[1]) and torch.equal(att, three[2])
    assert same(forward(m, d, True, monkeypatch), (prob, logit))  # without the attention output
    for name, got, ref in zip(("prob", "logit", "att"), fused, want):
        print(f"{c} {cell} {activation} bn={batch_norm} {name}: max |err| = "
              f"{(got.double().cpu() - ref).abs().max().item():.3e}")
    for got, ref in zip(fused, want):
        torch.testing.assert_close(got.double().cpu(), ref, **TOL)
    assert rankops.error_flags() == 0


@cells
@pytest.mark.parametrize("c", CASES, ids=lambda c: "B%d_T%d_H%d" % c)
def test_fused_forward_is_bit_equal_to_the_three_launches(c, cell, monkeypatch):
    check(c, cell, "dice", True, monkeypatch)


@cells
@pytest.mark.parametrize("activation,batch_norm", [("dice", False), ("prelu", True), ("prelu", False)])
def test_fused_forward_with_every_tail_epilogue(activation, batch_norm, cell, monkeypatch):
    check((16, 50, 16), cell, activation, batch_norm, monkeypatch)  # (dice, True) is the test above


@cells
def test_the_fused_launch_is_the_only_one(cell, monkeypatch):
    m, inp, d, want = setup((17, 50, 16), cell)
    three = forward(m, d, False, monkeypatch, return_attention=True)
    only_the_fused_launch(monkeypatch)
    got = forward(m, d, True, monkeypatch, return_attention=True)
    assert same(got, three)
    assert same(forward(m, d, True, monkeypatch), three[:2])
    assert rankops.error_flags() == 0


@cells
def test_poisoned_history_ids_past_the_length_change_nothing(cell, monkeypatch):
    c = (67, 50, 32)
    m, inp, d, want = setup(c, cell)
    clean = forward(m, d, True, monkeypatch, return_attention=True)
    lens = inp["sequence"][SEQ_LEN]
    past = torch.arange(c[1])[None, :] >= lens[:, None]
    only_the_fused_launch(monkeypatch)
    for poison in (H.SMALL_VOCAB["feedid"], H.SMALL_VOCAB["feedid"] + 5, -1, 2 ** 40):  # never read
        bad = inp["sequence"][SEQ].clone()
        bad[past] = poison
        seq = {SEQ: bad.cuda(), SEQ_LEN: d["sequence"][SEQ_LEN]}
        assert same(forward(m, dict(d, sequence=seq), True, monkeypatch, return_attention=True), clean), poison
        assert rankops.error_flags() == 0, poison


@pytest.mark.parametrize("where", ["history", "category", "target"])
def test_out_of_range_ids_read_zero_and_raise_the_flag(where, monkeypatch):
    c = (17, 50, 16)
    m, inp, d, want = setup(c, "AUGRU")
    clean = forward(m, d, True, monkeypatch, return_attention=True)
    bad = dict(d)
    if where == "history":
        r = int(torch.nonzero(inp["sequence"][SEQ_LEN] >= 5)[-1])  # a live step, late in the batch
        ids = d["sequence"][SEQ].clone()
        ids[r, 3] = H.SMALL_VOCAB["feedid"] + 1  # one past the last table row
        bad["sequence"] = {SEQ: ids, SEQ_LEN: d["sequence"][SEQ_LEN]}
    elif where == "category":
        r = 16  # the one row of the second workgroup
        ids = d["category"]["userid"].clone()
        ids[r] = -1
        bad["category"] = dict(d["category"], userid=ids)
    else:
        r = 5
        ids = d["target"]["feedid"].clone()
        ids[r] = 2 ** 33
        bad["target"] = {"feedid": ids}
    assert rankops.error_flags() == 0
    fused = forward(m, bad, True, monkeypatch, return_attention=True)
    assert rankops.error_flags() & _lib.RK_FLAG_INDEX_OOB  # reads and resets
    assert rankops.error_flags() == 0
    three = forward(m, bad, False, monkeypatch, return_attention=True)
    assert rankops.error_flags() & _lib.RK_FLAG_INDEX_OOB
    assert same(fused, three)
    assert not torch.equal(fused[1][r], clean[1][r])  # the zero row does change that sample
    keep = torch.ones(c[0], dtype=torch.bool, device="cuda")
    keep[r] = False
    assert torch.equal(fused[1][keep], clean[1][keep])


def test_past_one_workgroup_per_cu_forward_takes_the_three_launches(monkeypatch):
    m, inp, d, want = setup((17, 50, 16), "AGRU")  # two workgroups
    fused = forward(m, d, True, monkeypatch)
    monkeypatch.setattr(common, "_num_cus", lambda device: 1)
    with monkeypatch.context() as mp:
        mp.setattr(ops, "dien_forward", refuse("ops.dien_forward"))
        assert same(forward(m, d, True, monkeypatch), fused)
        mp.setattr(common, "FUSED_DIEN_WG_PER_CU", 2)
        with pytest.raises(AssertionError, match="ops.dien_forward was called"):
            forward(m, d, True, monkeypatch)
    only_the_fused_launch(monkeypatch)
    m16, _, d16, _ = setup((16, 50, 16), "AGRU")  # one workgroup: still the one launch
    assert len(forward(m16, d16, True, monkeypatch)) == 2


def inputs_of(d):
    return d["dense"], d["category"], d["sequence"], d["target"]


@pytest.mark.parametrize("B,T,Hd,nh", [(9, 3, 16, 16), (5, 200, 32, 8)], ids=["nh16", "T200_H32"])
def test_outside_the_envelope_forward_takes_the_three_launches_and_prepare_refuses(B, T, Hd, nh, monkeypatch):
    m, inp = make(B, T, Hd, "AGRU", nh=nh)
    m, d = m.cuda(), H.to_device(inp, "cuda")
    off = forward(m, d, False, monkeypatch, return_attention=True)
    on = forward(m, d, True, monkeypatch, return_attention=True)
    assert same(on, off)
    if nh == 8:  # the library refused (its LDS need: 16 slices of 200 x 32 floats) and the model remembers
        assert (m._tail[0].linear.in_features, T, Hd) in m._unfusable
        monkeypatch.setattr(ops, "dien_forward", refuse("ops.dien_forward"))
        assert same(forward(m, d, True, monkeypatch, return_attention=True), off)
    with pytest.raises(RuntimeError, match="envelope"):
        m.prepare(*inputs_of(d))
    want = dien_ref.forward(H.cpu_params(m), *inputs_of(inp))
    torch.testing.assert_close(on[1].double().cpu(), want[1], **TOL)
    assert rankops.error_flags() == 0


def test_prepare_runs_the_forward_on_the_current_inputs(monkeypatch):
    B, T, Hd = 17, 50, 16
    m, inp = make(B, T, Hd, "AUGRU")
    m, d = m.cuda(), H.to_device(inp, "cuda")
    run = m.prepare(*inputs_of(d))
    assert isinstance(run.plan, ops.DienPlan)
    want = forward(m, d, True, monkeypatch)
    other = H.to_device(make(B, T, Hd, "AUGRU", seed=77)[1], "cuda")
    with monkeypatch.context() as mp:
        only_the_fused_launch(mp)
        prob, logit = run()
        torch.cuda.synchronize()
        assert torch.equal(prob, want[0]) and torch.equal(logit, want[1])
        # the bound inputs change in place: a dense column, the target ids, the history ids and the lengths
        d["dense"]["videoplayseconds"].add_(0.5)
        d["target"]["feedid"].copy_(other["target"]["feedid"])
        d["sequence"][SEQ].copy_(other["sequence"][SEQ])
        d["sequence"][SEQ_LEN].copy_(other["sequence"][SEQ_LEN])
        again = run()
        torch.cuda.synchronize()
    assert again[0] is prob and again[1] is logit
    fresh = forward(m, d, False, monkeypatch)
    assert torch.equal(prob, fresh[0]) and torch.equal(logit, fresh[1])
    assert not torch.equal(logit, want[1])
    assert rankops.error_flags() == 0


def test_prepared_run_in_a_captured_graph_follows_its_inputs(monkeypatch):
    B, T, Hd = 17, 50, 16
    m, inp = make(B, T, Hd, "AGRU")
    m, d = m.cuda(), H.to_device(inp, "cuda")
    run = m.prepare(*inputs_of(d))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        prob, logit = run()
    seen = []
    for seed in (42, 91, 92):  # three replays, each over other inputs
        other = H.to_device(make(B, T, Hd, "AGRU", seed=seed)[1], "cuda")
        d["dense"]["u_like_7d_sum"].copy_(other["dense"]["u_like_7d_sum"])
        d["category"]["userid"].copy_(other["category"]["userid"])
        d["target"]["feedid"].copy_(other["target"]["feedid"])
        d["sequence"][SEQ].copy_(other["sequence"][SEQ])
        d["sequence"][SEQ_LEN].copy_(other["sequence"][SEQ_LEN])
        g.replay()
        torch.cuda.synchronize()
        fresh = forward(m, d, False, monkeypatch)
        assert torch.equal(prob, fresh[0]) and torch.equal(logit, fresh[1]), seed
        seen.append(logit.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert rankops.error_flags() == 0


def test_prepare_is_for_eval_mode(monkeypatch):
    m, inp = make(7, 3, 8, "AGRU")
    m, d = m.cuda(), H.to_device(inp, "cuda")
    with pytest.raises(RuntimeError, match="eval"):
        m.train().prepare(*inputs_of(d))
    run = m.eval().prepare(*inputs_of(d))
    assert same(run(), forward(m, d, False, monkeypatch))


def test_an_empty_batch_returns_empty_rows_without_a_launch(monkeypatch):
    m, inp, d, want = setup((7, 3, 8), "AGRU")
    none = H.to_device(H.din_inputs(0, 3, H.SMALL_VOCAB), "cuda")
    only_the_fused_launch(monkeypatch)
    monkeypatch.setattr(ops, "dien_forward", refuse("ops.dien_forward"))
    prob, logit = forward(m, none, True, monkeypatch)
    assert prob.shape == (0, 1) and logit.shape == (0, 1) and prob.dtype == torch.float32
