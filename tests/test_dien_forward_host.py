"""CPU tests of the one-launch DIEN forward's host side: rk_dien_forward / rk_dien_forward_plan validate
every argument before any launch (so they answer on a machine without a GPU), and the Python surface
(DIEN.prepare, the switch, the ops) is there."""
import ctypes

import pytest
import torch

import helpers as H
import rankops
from rankops import _lib, common, ops

INVALID, UNSUPPORTED = 1, _lib.RK_ERR_UNSUPPORTED  # RK_ERR_INVALID, include/rankops.h
ONE = 16  # any non-null, 16-B aligned address: validation never dereferences it


def segments(target_dim=16, target_col=50):
    """[50 dense columns | the target row]: one dense and one table segment."""
    segs = [_lib.Segment(ONE, None, 0, 50, 0, 50, 0), _lib.Segment(ONE, ONE, 1, target_dim, 10, target_dim, target_col)]
    return (_lib.Segment * 2)(*segs)


def layers(units=(512, 256, 128), width=74):
    out, k = [], width
    for n in units:
        out.append(_lib.MlpLayer(w=ONE, ldw=(k + 63) // 64 * 64, n=n))
        k = n
    return (_lib.MlpLayer * len(out))(*out)


def call(**change):
    """rk_dien_forward on a valid argument list (width 74 = 50 + H 16 + nh 8, T 5, an empty batch) with
    `change` applied; returns the code."""
    head = _lib.Epilogue(head_w=ONE, head_b=ONE)
    a = dict(row_segs=segments(), nseg=2, width=74, q_col=50, state_col=66, key_table=ONE, key_rows=10, ld_key=16,
             seq=ONE, ld_seq=5, T=5, seq_len=ONE, batch=0, H=16, nh=8, cell_type=0, Wg=ONE, bg=ONE, Wc=ONE, bc=ONE,
             A=ONE, Vg=ONE, vg=ONE, Vc=ONE, vc=ONE, layers=layers(), nlayers=3, head=ctypes.byref(head), att_out=None,
             ld_att=0, stream=None)
    assert set(change) <= set(a), change
    a.update(change)
    return _lib.load().rk_dien_forward(*a.values())


def test_a_valid_call_over_an_empty_batch_launches_nothing():
    assert call() == 0
    assert call(cell_type=1, att_out=ONE, ld_att=5) == 0


@pytest.mark.parametrize("name", ["row_segs", "key_table", "seq", "seq_len", "Wg", "bg", "Wc", "bc", "A", "Vg", "vg",
                                  "Vc", "vc", "layers", "head"])
def test_null_pointers_are_invalid(name):
    assert call(**{name: None}) == INVALID
    assert "rk_dien_forward" in _lib.last_error() and "null" in _lib.last_error()


def test_a_head_without_weights_is_invalid():
    assert call(head=ctypes.byref(_lib.Epilogue(head_b=ONE))) == INVALID


@pytest.mark.parametrize("change", [dict(cell_type=2), dict(cell_type=-1), dict(T=0), dict(batch=-1), dict(ld_seq=4),
                                    dict(ld_key=8), dict(key_rows=0), dict(att_out=ONE, ld_att=4), dict(nseg=0),
                                    dict(q_col=-1)], ids=str)
def test_bad_shapes_and_cells_are_invalid(change):
    assert call(**change) == INVALID


def test_row_layout_is_checked():
    assert call(row_segs=segments(target_dim=30)) == INVALID  # the target segment ends at column 80 > width
    assert "segment 1" in _lib.last_error()
    assert call(state_col=70) == INVALID  # state_col + nh > width
    assert "state columns" in _lib.last_error()
    assert call(q_col=60) == INVALID  # q_col + H > width
    assert call(state_col=60) == INVALID  # the state columns inside the query's


def test_outside_the_envelope_is_unsupported():
    lib = _lib.load()
    assert call(nh=16) == UNSUPPORTED  # its phases need more registers than a 1,024-thread workgroup allows
    assert "envelope" in _lib.last_error()
    assert call(H=12) == UNSUPPORTED
    assert call(T=257, ld_seq=257) == UNSUPPORTED
    assert call(key_table=20) == UNSUPPORTED and "aligned" in _lib.last_error()
    assert call(ld_key=18) == UNSUPPORTED
    assert call(layers=layers((256, 128)), nlayers=2) == UNSUPPORTED and "plan" in _lib.last_error()
    assert call(width=200, layers=layers(width=200)) == UNSUPPORTED
    assert call(row_segs=segments(), nseg=33) == UNSUPPORTED
    # T 200 at H 32: 16 slices of 200 rows of 32 floats are far past the CU's 160 KiB
    wide = dict(row_segs=segments(32), width=90, state_col=82, H=32, ld_key=32, layers=layers(width=90))
    assert call(**wide) == 0
    assert call(**wide, T=200, ld_seq=200) == UNSUPPORTED and "LDS" in _lib.last_error()
    assert lib.rk_dien_plan_launch(None, None) == INVALID


def test_a_plan_validates_like_the_call_and_an_empty_one_launches_nothing():
    lib = _lib.load()
    head = _lib.Epilogue(head_w=ONE, head_b=ONE)
    w9 = [ONE] * 9
    args = [segments(), 2, 74, 50, 66, ONE, 10, 16, ONE, 5, 5, ONE, 0, 16, 8, 1, *w9, layers(), 3, ctypes.byref(head),
            None, 0]
    assert lib.rk_dien_forward_plan(*args, None) == INVALID
    handle = ctypes.c_void_p()
    bad = list(args)
    bad[14] = 16  # nh
    assert lib.rk_dien_forward_plan(*bad, ctypes.byref(handle)) == UNSUPPORTED and not handle.value
    assert lib.rk_dien_forward_plan(*args, ctypes.byref(handle)) == 0 and handle.value
    assert lib.rk_dien_plan_launch(handle, None) == 0
    lib.rk_dien_plan_destroy(handle)
    lib.rk_dien_plan_destroy(None)


def test_the_python_surface_is_there():
    assert callable(rankops.DIEN.prepare)
    assert "binds the current weights" in " ".join(rankops.DIEN.prepare.__doc__.split())
    assert isinstance(common.FUSED_DIEN, bool) and common.FUSED_DIN is True
    assert common.FUSED_DIEN_WG_PER_CU == 1
    assert callable(ops.dien_forward) and callable(ops.dien_forward_plan) and callable(ops.DienPlan.launch)


def test_prepare_refuses_train_mode_and_cpu_tensors():
    m = rankops.DIEN(None, vocab_sizes=H.SMALL_VOCAB, trainable=True)
    inp = H.din_inputs(3, 6, H.SMALL_VOCAB)
    with pytest.raises(RuntimeError, match="eval"):
        m.train().prepare(inp["dense"], inp["category"], inp["sequence"], inp["target"])
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        m.eval().prepare(inp["dense"], inp["category"], inp["sequence"], inp["target"])
    assert torch.is_tensor(inp["target"]["feedid"])
