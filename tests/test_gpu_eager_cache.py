"""GPU: the eager eval forwards through common.EagerCalls (cached marshalled launches, fresh outputs
per call) equal the uncached path bit for bit, follow new input contents in the same buffers,
rebuild on new buffers, shapes and parameter updates, keep earlier outputs intact, and keep the
per-call H2 draw sequence (dcn.py:37-45, din.py:61-67) — checked against the oracle."""
import pytest
import torch

import helpers as H
from rankops import common

MODELS = {
    "dcn": {"vocab": H.WECHAT_VOCAB, "interaction_weights": "frozen"},
    "din": {"vocab": H.WECHAT_VOCAB, "T": 50, "dim": 32, "interaction_weights": "frozen"},
    "deepfm": {"dim": 32, "fields": {f"f{i:02d}": 5000 + i for i in range(30)}},
    "fwfm": {"vocab": H.WECHAT_VOCAB, "dim": 8},
}


def _run(model, name, inp, cached):
    prev = common.EAGER_CACHE
    common.EAGER_CACHE = cached
    try:
        with torch.no_grad():
            out = H.as_tuple(H.call_model(model, name, inp))
        torch.cuda.synchronize()
        return tuple(o.clone() if isinstance(o, torch.Tensor) else o for o in out), out
    finally:
        common.EAGER_CACHE = prev


def _equal(a, b):
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert torch.equal(x, y)
        else:
            assert x == y


def _copy_into(dst, src):
    if isinstance(dst, dict):
        for k in dst:
            _copy_into(dst[k], src[k])
    else:
        dst.copy_(src)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MODELS))
def test_cached_eager_equals_uncached_and_follows_inputs(name):
    cfg = MODELS[name]
    model = H.build(name, cfg).cuda().eval()
    inp = H.to_device(H.make_inputs(name, cfg, 1000, seed=5), "cuda")
    ref, _ = _run(model, name, inp, cached=False)
    a, a_live = _run(model, name, inp, cached=True)   # builds the entry
    b, b_live = _run(model, name, inp, cached=True)   # hit
    _equal(a, ref)
    _equal(b, ref)
    assert a_live[0].data_ptr() != b_live[0].data_ptr() or a_live[0] is not b_live[0]
    assert torch.equal(a_live[0], a[0])  # the earlier output was not overwritten by the hit
    assert len(model.__dict__["_eager"]) >= 1
    # new contents in the same buffers: the cached launch reads them
    new = H.to_device(H.make_inputs(name, cfg, 1000, seed=6), "cuda")
    _copy_into(inp, new)
    c, _ = _run(model, name, inp, cached=True)
    d, _ = _run(model, name, new, cached=False)
    _equal(c, d)
    assert not torch.equal(c[0], a[0])
    # other buffers and another batch size: new entries
    e, _ = _run(model, name, new, cached=True)
    _equal(e, d)
    small = H.to_device(H.make_inputs(name, cfg, 37, seed=7), "cuda")
    f, _ = _run(model, name, small, cached=True)
    g, _ = _run(model, name, small, cached=False)
    _equal(f, g)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MODELS))
def test_cached_eager_rebuilds_after_parameter_updates(name):
    cfg = MODELS[name]
    model = H.build(name, cfg).cuda().eval()
    inp = H.to_device(H.make_inputs(name, cfg, 300, seed=8), "cuda")
    before, _ = _run(model, name, inp, cached=True)
    with torch.no_grad():  # an optimizer-style in-place update of every parameter
        for p in model.parameters():
            p.mul_(0.9).add_(0.01)
    after, _ = _run(model, name, inp, cached=True)
    want, _ = _run(model, name, inp, cached=False)
    _equal(after, want)
    assert not torch.equal(after[0], before[0])
    # a state_dict round trip (copies into the same storages) and .train()/.eval()
    sd = {k: v.clone() for k, v in H.build(name, cfg, seed=3).state_dict().items()}
    model.load_state_dict(sd)
    model.train().eval()
    x, _ = _run(model, name, inp, cached=True)
    y, _ = _run(model, name, inp, cached=False)
    _equal(x, y)


BOUND_MODELS = dict(MODELS, afm={}, bst={"T": 20, "dim": 16}, deepcrossing={"interaction_weights": "frozen"})
# the C entry points one forward issues: (cached eager hit, prepared run()), recorded once on the
# commit before the eval forwards moved onto common.Bound, and equal to the model docstrings' launches
BOUND_LAUNCHES = {
    "afm": (["rk_afm_forward"], ["rk_afm_forward"]),
    "bst": (["rk_bst_small_forward"], ["rk_bst_small_forward"]),
    "dcn": (["rk_dcn_forward"], ["rk_dcn_forward"]),
    "deepcrossing": (["rk_mlp_forward_gather"], ["rk_mlp_forward_gather"]),
    "deepfm": (["rk_deepfm_forward"], ["rk_deepfm_forward"]),
    "din": (["rk_din_forward_ex"], ["rk_din_plan_launch"]),
    "fwfm": (["rk_fwfm_forward"], ["rk_fwfm_forward"]),
}


class _Recorder:
    """The library handle with every call's entry-point name noted."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


def _prepare(model, name, inp):
    if name in ("dcn", "deepcrossing"):
        return model.prepare(inp["dense"], inp["category"])
    if name == "din":
        return model.prepare(inp["dense"], inp["category"], inp["sequence"], inp["target"])
    if name == "afm":
        return model.prepare(inp["dense_input"], inp["category_input"])
    if name == "bst":
        return model.prepare(inp["dense"], inp["category"], inp["seq_feedid"], inp["seq_length"])
    return model.prepare(inp["category"] if name == "deepfm" else inp["x"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BOUND_MODELS))
def test_hit_uncached_and_prepared_agree_and_issue_the_same_launches(name, monkeypatch):
    """One bound eval forward per model: the cached eager hit, the forward with EAGER_CACHE off and
    prepare()'s run() return bit-identical outputs, and the hit and run() issue exactly the C entry
    points of BOUND_LAUNCHES.  Batch 37: two full 16-row tiles and a 5-row remainder."""
    from rankops import ops
    cfg = BOUND_MODELS[name]
    model = H.build(name, cfg).cuda().eval()
    inp = H.to_device(H.make_inputs(name, cfg, 37, seed=12), "cuda")
    rec = _Recorder(ops._lib.load())
    monkeypatch.setattr(ops._lib, "load", lambda: rec)
    _run(model, name, inp, cached=True)  # builds the entry (and draws the frozen H2 weights)
    rec.names.clear()
    hit, _ = _run(model, name, inp, cached=True)
    hit_names = list(rec.names)
    uncached, _ = _run(model, name, inp, cached=False)
    with torch.no_grad():
        run = _prepare(model, name, inp)
        rec.names.clear()
        prepared = H.as_tuple(run())
        run_names = list(rec.names)
    torch.cuda.synchronize()
    assert len(prepared) >= len(hit) == len(uncached) >= 1
    _equal(hit, uncached)
    _equal(hit, prepared[:len(hit)])  # FwFM: forward() returns prob alone, run() (prob, logit)
    assert (hit_names, run_names) == BOUND_LAUNCHES[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dcn", "din"])
def test_cached_eager_per_call_draws_match_oracle(name):
    """Per-call H2 weights: every cached forward still draws from the CPU generator in the
    reference's order, once per forward."""
    cfg = dict(MODELS[name], interaction_weights="per_call")
    model = H.build(name, cfg)
    p = H.cpu_params(model)
    inp = H.make_inputs(name, cfg, 200, seed=9)
    model = model.cuda().eval()
    d = H.to_device(inp, "cuda")
    torch.manual_seed(11)
    with torch.no_grad():
        outs = [H.as_tuple(H.call_model(model, name, d)) for _ in range(3)]
    torch.manual_seed(11)
    with torch.no_grad():
        refs = [H.as_tuple(H.call_oracle(name, cfg, p, inp)) for _ in range(3)]
    for o, r in zip(outs, refs):
        for x, y in zip(o, r):
            if isinstance(y, torch.Tensor):
                torch.testing.assert_close(x.cpu(), y, atol=1e-4, rtol=1e-4)
