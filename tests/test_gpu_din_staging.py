"""GPU: the staging and the l2 hand-off of din_forward_kernel (din_fused.hip).  The attention
weights reach LDS from the packed image or split in the kernel, and the streamed phase B runs the
l2 hand-off (a chain of agent-scope atomics) in an idle wave beside its last layer.  Neither
changes any arithmetic: the outputs match the oracle, the balanced and the contiguous
assignment agree bit for bit at the batch sizes where a workgroup or a universe is nearly empty,
the launch without the image agrees bit for bit, and the l2 term survives launches issued back to
back and graph replays."""
import pytest
import torch

import helpers as H
from rankops import common

ATOL = RTOL = 1e-4  # the project's DIN tolerance (tests/test_gpu_din_plan.py)
VOCAB = {"userid": 200, "feedid": 200, "device": 2, "authorid": 200, "bgm_song_id": 200, "bgm_singer_id": 200,
         "manual_tag_list": 200}
LEN_KEY = "his_read_comment_7d_seq_length"
SEQ_KEY = "his_read_comment_7d_seq"


def _cfg(**kw):
    cfg = {"vocab": VOCAB, "T": 50, "dim": 32, "interaction_weights": "frozen"}
    cfg.update(kw)
    return cfg


def _inputs(cfg, batch, seed):
    """Lengths 0, 1, 16, 17, T and T + 5 lead every batch that has room for them."""
    inp = H.make_inputs("din", cfg, batch, seed=seed)
    T = cfg["T"]
    edge = torch.tensor([0, 1, 16, 17, T, T + 5])
    if batch >= len(edge):
        inp["sequence"][LEN_KEY][: len(edge)] = edge
    return inp


def _clone(out):
    return tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in H.as_tuple(out))


@pytest.mark.gpu
@pytest.mark.parametrize("softmax", [False, True])
@pytest.mark.parametrize("T", [16, 33, 50])
@pytest.mark.parametrize("dim", [8, 16, 32])
def test_oracle_and_cross_assignment_equality(monkeypatch, dim, T, softmax):
    """Prepared plan and eager forward against the oracle (H 8 / 16 / 32: attention images of 18 /
    24 / 36 KiB), and balanced against contiguous launches bit for bit (l2 within fp32 rounding:
    the workgroups' partial sums group the rows differently), at batches 1, 16, 17 (a second workgroup with one row), 33 and 1041 (a second universe of 17)."""
    cfg = _cfg(dim=dim, T=T, softmax=softmax)
    model = H.build("din", cfg)
    p = H.cpu_params(model)
    model = model.cuda().eval()
    first = True
    for batch in (1, 16, 17, 33, 1041):
        inp = _inputs(cfg, batch, seed=7 * batch + dim + T)
        d = H.to_device(inp, "cuda")
        args = (d["dense"], d["category"], d["sequence"], d["target"])
        with torch.no_grad():
            monkeypatch.setenv("RANKOPS_DIN_BALANCE", "1")
            if first:
                torch.manual_seed(5)  # the frozen H2 draw happens on the first forward
                first = False
            plan = _clone(model.prepare(*args)())
            eager = _clone(H.call_model(model, "din", d))
            monkeypatch.setenv("RANKOPS_DIN_BALANCE", "0")
            ctg = _clone(H.call_model(model, "din", d))
            torch.manual_seed(5)  # the oracle draws per call
            ref = H.as_tuple(H.call_oracle("din", cfg, p, inp))
        torch.cuda.synchronize()
        for name, got in (("plan", plan), ("eager", eager)):
            assert len(got) == len(ref) == 3
            for i, (g, r) in enumerate(zip(got, ref)):
                torch.testing.assert_close(g.cpu().reshape(r.shape), r, atol=ATOL, rtol=RTOL,
                                           msg=lambda m: f"batch {batch} {name} output {i}: {m}")
            assert torch.equal(got[0], ctg[0]) and torch.equal(got[1], ctg[1]), (batch, name)
            torch.testing.assert_close(got[2], ctg[2], rtol=1e-6, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("softmax", [False, True])
def test_without_attention_image_bit_identical(monkeypatch, softmax):
    """rk_din_forward without att_image (the legacy staging: the split formed in the kernel from
    w1..w3) equals the launch with the packed image bit for bit: batch 33, H 32, T 50."""
    cfg = _cfg(softmax=softmax)
    model = H.build("din", cfg).cuda().eval()
    d = H.to_device(_inputs(cfg, 33, seed=33), "cuda")
    monkeypatch.setenv("RANKOPS_DIN_BALANCE", "1")
    monkeypatch.setattr(common, "EAGER_CACHE", False)  # the plain rk_din_forward call
    with torch.no_grad():
        with_image = _clone(H.call_model(model, "din", d))
        monkeypatch.setattr(model, "_att_image", lambda w, Hdim: None)
        without = _clone(H.call_model(model, "din", d))
    torch.cuda.synchronize()
    assert len(with_image) == len(without) == 3
    for a, b in zip(with_image, without):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("softmax", [False, True])
@pytest.mark.parametrize("batch", [16, 17, 1040])
def test_l2_over_repeated_launches_and_graph_replays(monkeypatch, batch, softmax):
    """30 launches of one prepared plan with no sync between them, for grids of 1, 2 and 65
    workgroups, then the same plan captured in a graph and replayed 30 times: the last launch's
    l2 equals the l2 of one synchronised eager launch (the same workgroup partials summed in the
    reader's fixed lane order, so fp32 rounding at most: rtol 1e-6, as
    test_l2_hand_off_stable_over_repeated_launches) and the oracle's within the DIN tolerance."""
    cfg = _cfg(softmax=softmax)
    model = H.build("din", cfg)
    p = H.cpu_params(model)
    model = model.cuda().eval()
    inp = _inputs(cfg, batch, seed=batch)
    d = H.to_device(inp, "cuda")
    monkeypatch.setenv("RANKOPS_DIN_BALANCE", "1")
    args = (d["dense"], d["category"], d["sequence"], d["target"])
    with torch.no_grad():
        torch.manual_seed(5)
        want = _clone(H.call_model(model, "din", d))
        torch.cuda.synchronize()
        torch.manual_seed(5)
        ref = H.as_tuple(H.call_oracle("din", cfg, p, inp))
        torch.testing.assert_close(want[2].cpu().reshape(ref[2].shape), ref[2], atol=ATOL, rtol=RTOL)
        run = model.prepare(*args)
        for _ in range(30):
            out = run()
        torch.cuda.synchronize()
        torch.testing.assert_close(out[2], want[2], rtol=1e-6, atol=0)
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
        out[2].fill_(float("nan"))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run()
        out[2].fill_(float("nan"))
        for _ in range(30):
            graph.replay()
        torch.cuda.synchronize()
        torch.testing.assert_close(out[2], want[2], rtol=1e-6, atol=0)
        assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("softmax", [False, True])
def test_plan_follows_inputs_overwritten_in_place(monkeypatch, softmax):
    """A plan launched, its inputs overwritten in place, launched again: the outputs follow the
    inputs (every load, the image's included, happens at launch, none at prepare)."""
    cfg = _cfg(softmax=softmax)
    model = H.build("din", cfg).cuda().eval()
    monkeypatch.setenv("RANKOPS_DIN_BALANCE", "1")
    d = H.to_device(_inputs(cfg, 33, seed=1), "cuda")
    with torch.no_grad():
        run = model.prepare(d["dense"], d["category"], d["sequence"], d["target"])
        out1 = _clone(run())
        new = H.to_device(_inputs(cfg, 33, seed=2), "cuda")
        d["sequence"][SEQ_KEY].copy_(new["sequence"][SEQ_KEY])
        d["sequence"][LEN_KEY].copy_(new["sequence"][LEN_KEY])
        d["target"]["feedid"].copy_(new["target"]["feedid"])
        for k in d["category"]:
            d["category"][k].copy_(new["category"][k])
        out2 = _clone(run())
        eager2 = _clone(H.call_model(model, "din", d))
    torch.cuda.synchronize()
    for a, b in zip(out2, eager2):
        assert torch.equal(a, b)
    assert not torch.equal(out2[0], out1[0])
