"""CPU tests of DIEN training's host side: the opt-in `trainable` flag of rankops.DIEN, and the
float64 restatement's autograd, which tests/test_gpu_dien_train.py uses as its oracle."""
import inspect

import pytest
import torch

import dien_ref
import helpers as H
import rankops


def make(**kw):
    return rankops.DIEN(None, vocab_sizes=H.SMALL_VOCAB, **kw)


def test_trainable_is_keyword_only_and_off_by_default():
    prm = inspect.signature(rankops.DIEN.__init__).parameters["trainable"]
    assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default is False
    assert make().trainable is False and make(trainable=True).trainable is True


def test_parameters_and_initialisation_do_not_depend_on_the_flag():
    torch.manual_seed(9)
    a = make(custom_gru_type="AUGRU").state_dict()
    torch.manual_seed(9)
    b = make(custom_gru_type="AUGRU", trainable=True).state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_default_model_still_raises_in_train_mode():
    inp = H.din_inputs(4, 8, H.SMALL_VOCAB)
    with pytest.raises(NotImplementedError):
        make().train()(inp["dense"], inp["category"], inp["sequence"], inp["target"])


def test_trainable_model_refuses_cpu_inputs():
    inp = H.din_inputs(4, 8, H.SMALL_VOCAB)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        make(trainable=True).train()(inp["dense"], inp["category"], inp["sequence"], inp["target"])


@pytest.mark.parametrize("cell", ["AGRU", "AUGRU"])
def test_restatement_autograd_gives_zero_key_gradients_past_the_length(cell):
    B, T, Hd, nh = 5, 7, 8, 8
    g = torch.Generator().manual_seed(17)
    q = torch.randn(B, Hd, generator=g, dtype=torch.float64).requires_grad_(True)
    keys = torch.randn(B, T, Hd, generator=g, dtype=torch.float64).requires_grad_(True)
    lens = torch.tensor([0, 1, T, 3, 5])
    w = [t.double().requires_grad_(True) for t in dien_ref.draw_weights(Hd, nh, 18)]
    s, _, _ = dien_ref.interest(q, keys, lens, w, cell)
    (s * torch.randn(B, nh, generator=g, dtype=torch.float64)).sum().backward()
    past = torch.arange(T)[None, :] >= lens[:, None]
    assert float(keys.grad[past].abs().max()) == 0.0
    assert float(keys.grad[~past].abs().min()) > 0.0
    # the query acts through the softmax only: nothing for len 0, and a single position has weight 1
    assert float(q.grad[:2].abs().max()) == 0.0 and float(q.grad[2:].abs().min()) > 0.0
    if cell == "AGRU":  # the update gate never reaches the output
        assert float(w[5].grad[nh:].abs().max()) == 0.0 and float(w[6].grad[nh:].abs().max()) == 0.0
