"""CPU tests of what rankops.MMoE and rankops.PLE share (their common base class): the modules each
constructor creates, in order, with the seeded values, against a snapshot recorded before the two
classes shared any code (tests/golden/multitask_state.json: state_dict keys in order, shapes, and the
exact sum of every tensor), and the text of the errors both raise, which carry the model's name."""
import json
import math
import os

import pytest
import torch

import rankops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multitask_state.json")
VOCAB = {"userid": 11, "feedid": 13, "device": 3, "authorid": 7, "bgm_song_id": 5, "bgm_singer_id": 6,
         "manual_tag_list": 9}
SMALL = dict(expert_hidden_units=(24, 12), task_names=("a", "b"), vocab_sizes=VOCAB)
CONFIGS = {
    "mmoe_two_tower_layers_no_dropout": lambda: rankops.MMoE(None, num_experts=3, tower_hidden_units=(10, 6),
                                                             dropout_rate=0, **SMALL),
    "ple_two_levels_shared_only": lambda: rankops.PLE(None, num_levels=2, num_specific_experts=0,
                                                      tower_hidden_units=(10,), **SMALL),
    "ple_two_levels": lambda: rankops.PLE(None, num_levels=2, tower_hidden_units=(10,), **SMALL),
}


def snapshot(name):
    """[key, shape, sum] per state_dict entry; the sum is math.fsum over float64, exact in any order."""
    torch.manual_seed(0)
    model = CONFIGS[name]()
    return [[k, list(v.shape), math.fsum(v.double().flatten().tolist())] for k, v in model.state_dict().items()]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_state_dict_matches_the_recorded_snapshot(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = snapshot(name)
    assert [g[0] for g in got] == [w[0] for w in want]
    assert got == want


HIDDEN = ("expert_hidden_units must be a non-empty list of positive widths and tower_hidden_units a list of "
          "positive widths, got {!r}, {!r}")
SHARED_ERRORS = [
    (dict(expert_hidden_units=()), HIDDEN.format((), (64,))),
    (dict(expert_hidden_units=(16, 0)), HIDDEN.format((16, 0), (64,))),
    (dict(tower_hidden_units=(-1,)), HIDDEN.format((256, 128), (-1,))),
    (dict(task_names=()), "task_names must be a non-empty list of distinct names, got ()"),
    (dict(task_names=("a", "a")), "task_names must be a non-empty list of distinct names, got ('a', 'a')"),
    (dict(dropout_rate=1.0), "dropout_rate must lie in [0, 1), got 1.0"),
    (dict(dropout_rate=-0.5), "dropout_rate must lie in [0, 1), got -0.5"),
]
OWN_ERRORS = {
    "MMoE": [(dict(num_experts=0), "num_experts must be positive, got 0")],
    "PLE": [(dict(num_levels=0), "num_levels must be positive, got 0"),
            (dict(num_specific_experts=-1),
             "num_specific_experts must be >= 0 and num_shared_experts >= 1, got -1, 2"),
            (dict(num_shared_experts=0),
             "num_specific_experts must be >= 0 and num_shared_experts >= 1, got 2, 0")],
}


@pytest.mark.parametrize("cls", ["MMoE", "PLE"])
def test_constructor_error_messages(cls):
    for kw, text in OWN_ERRORS[cls] + SHARED_ERRORS:
        with pytest.raises(ValueError) as e:
            getattr(rankops, cls)(None, vocab_sizes=VOCAB, **kw)
        assert str(e.value) == text, kw


@pytest.mark.parametrize("cls", ["MMoE", "PLE"])
def test_category_error_messages(cls):
    torch.manual_seed(0)
    model = getattr(rankops, cls)(None, **SMALL)
    ids = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(TypeError) as e:
        model._indices([ids])
    assert str(e.value) == f"{cls}.forward: category must be a dict of index tensors, got list"
    with pytest.raises(KeyError) as e:
        model._indices({"userid": ids, "device": ids})
    assert e.value.args[0] == (f"{cls}.forward: category features missing: "
                               "['authorid', 'bgm_song_id', 'bgm_singer_id', 'manual_tag_list']")
