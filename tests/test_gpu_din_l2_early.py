"""GPU: the l2 hand-off of din_forward_kernel as side steps of the streamed phase B (din_fused.hip
DinRowsReady, mlp_stream.h side steps).  The last wave publishes the workgroup's partial when phase B
opens, counts it a few chunks later, and the workgroup that counted last reads the partials, writes
the mean and resets the counter while the second fcn layer is still running.  The arithmetic and the
protocol are those of the hand-off behind the head, so: prob and logit of a prepared launch equal the
eager forward bit for bit and l2 within fp32 rounding (the project's bound for eager against plan,
rtol 1e-6); all match the oracle within the DIN tolerance; every one of a run of launches issued back
to back writes the same l2 bits (a counter reset too early or too late would show in one of them);
the launch without the l2 term gives the same prob and logit; and two plans with workspaces of their
own keep their values when they alternate on one stream.
Grids: batches 16, 17, 1041 and 2049 are 1, 2, 66 and 129 workgroups: one and two lanes of the reader
used, a second pass of its lane loop (66 > 64) and a third for lane 0 only (129), each time with a last
workgroup of one row (its last wave has no sample but runs every step).  H 32 / T 50 balanced and
contiguous, and H 8 / T 20 (another count of layer-0 chunks ahead of the phase-A barrier)."""
import pytest
import torch

import helpers as H

ATOL = RTOL = 1e-4  # the project's DIN tolerance (tests/test_gpu_din_plan.py)
VOCAB = {"userid": 200, "feedid": 200, "device": 2, "authorid": 200, "bgm_song_id": 200, "bgm_singer_id": 200,
         "manual_tag_list": 200}
LEN_KEY = "his_read_comment_7d_seq_length"
CASES = {"h32_balanced": (32, 50, "1"), "h32_contiguous": (32, 50, "0"), "h8_t20": (8, 20, "1")}
BATCHES = (16, 17, 1041, 2049)
LAUNCHES = 30

_models = {}
_contexts = {}


def _clone(out):
    return tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in H.as_tuple(out))


def _model(dim, T):
    if (dim, T) not in _models:
        cfg = {"vocab": VOCAB, "T": T, "dim": dim, "interaction_weights": "frozen"}
        model = H.build("din", cfg)
        p = H.cpu_params(model)
        _models[(dim, T)] = (cfg, model.cuda().eval(), p, [True])
    return _models[(dim, T)]


def _context(monkeypatch, case, batch):
    """Model, inputs, one synchronised eager forward, the oracle's and a prepared plan with its first
    launch's outputs: computed once per (case, batch) and left unchanged."""
    dim, T, balance = CASES[case]
    monkeypatch.setenv("RANKOPS_DIN_BALANCE", balance)
    key = (case, batch)
    if key in _contexts:
        return _contexts[key]
    cfg, model, p, first = _model(dim, T)
    inp = H.make_inputs("din", cfg, batch, seed=11 * batch + dim)
    edge = torch.tensor([0, 1, 16, 17, T, T + 5])  # lengths at the tile edges, as test_gpu_din_staging.py
    inp["sequence"][LEN_KEY][: len(edge)] = edge
    d = H.to_device(inp, "cuda")
    args = (d["dense"], d["category"], d["sequence"], d["target"])
    with torch.no_grad():
        if first[0]:
            torch.manual_seed(5)  # the frozen H2 draw happens on the model's first forward
            first[0] = False
        eager = _clone(H.call_model(model, "din", d))
        torch.manual_seed(5)  # the oracle draws per call
        ref = H.as_tuple(H.call_oracle("din", cfg, p, inp))
        run = model.prepare(*args)
        plan = _clone(run())
    torch.cuda.synchronize()
    _contexts[key] = dict(model=model, args=args, eager=eager, ref=ref, run=run, plan=plan)
    return _contexts[key]


def _bits(x):
    return x.detach().reshape(-1).view(torch.int32).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("case", list(CASES))
def test_launch_equals_eager_and_oracle(monkeypatch, case, batch):
    c = _context(monkeypatch, case, batch)
    plan, eager, ref = c["plan"], c["eager"], c["ref"]
    assert len(plan) == len(eager) == len(ref) == 3
    assert torch.equal(plan[0], eager[0]) and torch.equal(plan[1], eager[1])
    torch.testing.assert_close(plan[2], eager[2], rtol=1e-6, atol=0)
    for name, got in (("plan", plan), ("eager", eager)):
        for i, (g, r) in enumerate(zip(got, ref)):
            torch.testing.assert_close(g.cpu().reshape(r.shape), r, atol=ATOL, rtol=RTOL,
                                       msg=lambda m: f"{case} batch {batch} {name} output {i}: {m}")


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("case", list(CASES))
def test_every_launch_writes_the_same_l2(monkeypatch, case, batch):
    """30 launches with no synchronisation between them, l2_out filled with NaN before each launch
    and copied out after it (both stream-ordered); then the same through a captured graph of 5
    launches replayed 6 times.  All 30 values of each run are the bits of the plan's first launch."""
    c = _context(monkeypatch, case, batch)
    run, want = c["run"], c["plan"]
    out = run()
    torch.cuda.synchronize()
    got = torch.zeros(LAUNCHES, device="cuda")
    for i in range(LAUNCHES):
        out[2].fill_(float("nan"))
        run()
        got[i].copy_(out[2])
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want[2]).expand(LAUNCHES)), got
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])

    per, replays = 5, LAUNCHES // 5
    part = torch.zeros(per, device="cuda")
    got = torch.zeros(replays, per, device="cuda")

    def body():
        for i in range(per):
            out[2].fill_(float("nan"))
            run()
            part[i].copy_(out[2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    part.zero_()
    for r in range(replays):
        graph.replay()
        got[r].copy_(part)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want[2]).expand(LAUNCHES)), got
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("case", list(CASES))
def test_without_the_l2_term(monkeypatch, case, batch):
    """The prepared launch with l2_out == nullptr (the module's l2 term switched off): prob and logit
    are the bits of the launch with it."""
    c = _context(monkeypatch, case, batch)
    model = c["model"]
    monkeypatch.setattr(model, "mini_batch_aware_regularization", False)
    with torch.no_grad():
        run = model.prepare(*c["args"])
        off = _clone(run())
        off2 = _clone(run())
    torch.cuda.synchronize()
    assert not isinstance(off[2], torch.Tensor) and off[2] == 0.0
    for o in (off, off2):
        assert torch.equal(o[0], c["plan"][0]) and torch.equal(o[1], c["plan"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_two_plans_alternate_on_one_stream(monkeypatch, case):
    """Plans of batches 17 and 2049 (2 and 129 workgroups, a workspace and a counter each) launched in
    turn for 10 rounds with no synchronisation: each launch's l2 is the bits of the plan alone."""
    small, large = _context(monkeypatch, case, 17), _context(monkeypatch, case, 2049)
    rounds = 10
    got = torch.zeros(2, rounds, device="cuda")
    for r in range(rounds):
        for k, c in enumerate((small, large)):
            out = c["run"]()
            got[k, r].copy_(out[2])
            out[2].fill_(float("nan"))
    torch.cuda.synchronize()
    for k, c in enumerate((small, large)):
        assert torch.equal(_bits(got[k]), _bits(c["plan"][2]).expand(rounds)), (k, got[k])
        out = c["run"]()
        torch.cuda.synchronize()
        assert torch.equal(out[0], c["plan"][0]) and torch.equal(out[1], c["plan"][1])
