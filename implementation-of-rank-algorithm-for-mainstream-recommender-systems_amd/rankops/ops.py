"""Thin Python wrappers over the rankops C ABI.

Each wrapper validates devices/dtypes/shapes, turns tensors into device pointers and launches
on the current HIP stream of the tensors' device.  Outputs are allocated from PyTorch's
caching allocator, so every wrapper is safe inside `torch.cuda.graph` capture.  There is no
CPU path: a CPU tensor is an error (the CPU restatement in oracle/ is test-only).
"""
from __future__ import annotations

import ctypes
import os

import torch

from . import _lib
from ._lib import Epilogue, Segment, check, fptr, ptr

ACT = {"none": _lib.RK_ACT_NONE, "relu": _lib.RK_ACT_RELU, "leaky": _lib.RK_ACT_LEAKY,
       "dice": _lib.RK_ACT_DICE, "prelu": _lib.RK_ACT_PRELU}


def require_gpu(t: torch.Tensor, what: str):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"rankops: {what} must be a tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(
            f"rankops: {what} is on {t.device}; the rankops forward runs only on a ROCm GPU "
            f"(move the model and inputs with .to('cuda'))")
    return t


def as_index(t: torch.Tensor, what: str) -> torch.Tensor:
    require_gpu(t, what)
    if t.dtype != torch.int64:
        if t.dtype in (torch.int32, torch.int16, torch.uint8, torch.int8):
            t = t.long()
        else:
            raise TypeError(f"rankops: {what} must be an integer tensor, got {t.dtype}")
    return t


def bound_index(t: torch.Tensor, what: str, contiguous: bool = False) -> torch.Tensor:
    """An index tensor a prepared launch binds by address (Model.prepare): it must be the caller's
    own int64 tensor (and contiguous where the kernel reads it as a dense block), since a converted
    copy would silently stop following later writes to the caller's tensor."""
    require_gpu(t, what)
    if t.dtype != torch.int64:
        raise TypeError(f"rankops: prepare() binds {what} by address; it must be int64 (got {t.dtype}): "
                        "convert it once and pass the converted tensor")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"rankops: prepare() binds {what} by address; it must be contiguous")
    return t


def as_f32(t: torch.Tensor, what: str) -> torch.Tensor:
    require_gpu(t, what)
    if t.dtype != torch.float32:
        raise TypeError(f"rankops: {what} must be float32, got {t.dtype}")
    return t


def table_segment(weight: torch.Tensor, idx: torch.Tensor, out_col: int, idx_stride: int = None) -> Segment:
    """Embedding-table segment: rows weight[idx[b]] -> out[b, out_col:out_col+dim]."""
    if weight.dim() != 2 or weight.stride(1) != 1:
        raise ValueError("rankops: embedding weight must be 2-D with unit column stride")
    if idx_stride is None:
        if idx.dim() != 1:
            raise ValueError(f"rankops: expected a 1-D index tensor, got shape {tuple(idx.shape)}")
        idx_stride = idx.stride(0)
    return Segment(weight.data_ptr(), idx.data_ptr(), idx_stride, weight.stride(0), weight.shape[0],
                   weight.shape[1], out_col)


def packed_segment(packed: torch.Tensor, idx: torch.Tensor, dim: int, out_col: int) -> Segment:
    """Packed FM-table segment (rk_fm_gather_packed): row packed[idx[b]], D floats + weight at D."""
    if idx.dim() != 1 or idx.stride(0) != 1:
        raise ValueError("rankops: packed FM gather needs unit-stride 1-D indices")
    return Segment(packed.data_ptr(), idx.data_ptr(), 1, packed.stride(0), packed.shape[0], dim, out_col)


def dense_segment(src: torch.Tensor, dim: int, out_col: int, col_offset: int = 0) -> Segment:
    """Dense segment: src[b, col_offset:col_offset+dim] -> out[b, out_col:+dim] (src is [B] or [B, *])."""
    if src.dim() == 1:
        if dim != 1:
            raise ValueError("rankops: a 1-D dense source has dim 1")
        ld = src.stride(0)
    else:
        if src.stride(-1) != 1:
            raise ValueError("rankops: dense source must have unit column stride")
        ld = src.stride(0)
    return Segment(fptr(src, col_offset), None, 0, ld, 0, dim, out_col)


def _seg_array(segs):
    arr = (Segment * len(segs))(*segs)
    return arr


_SEG_ARRAYS = {}


def table_seg_array(weights, idxs, cols):
    """The rk_segment array of table segments weights[k][idxs[k]] -> column cols[k], memoized on
    every field of the structs (pointers, strides, shapes): a repeated training step, whose tables,
    index tensors and (recycled) gradient buffers come back at the same addresses, reuses the
    marshalled array instead of building a ctypes struct per field.  The library copies the array
    into the kernel arguments at launch, so sharing it is safe."""
    key = tuple((w.data_ptr(), w.stride(0), w.shape[0], w.shape[1], w.stride(1), i.data_ptr(), i.stride(0), i.dim(), c)
                for w, i, c in zip(weights, idxs, cols))
    arr = _SEG_ARRAYS.get(key)
    if arr is None:
        arr = _seg_array([table_segment(w, i, c) for w, i, c in zip(weights, idxs, cols)])
        if len(_SEG_ARRAYS) >= 512:
            _SEG_ARRAYS.clear()
        _SEG_ARRAYS[key] = arr
    return arr


def dense_table_seg_array(dense, ndense, weights, idxs):
    """[dense columns 0..ndense) + table segments side by side] as a memoized rk_segment array
    (DCN / DeepCrossing feature rows; table_seg_array's rules)."""
    key = (dense.data_ptr(), dense.stride(0), dense.dim(), ndense) + tuple(
        (w.data_ptr(), w.stride(0), w.shape[0], w.shape[1], w.stride(1), i.data_ptr(), i.stride(0), i.dim())
        for w, i in zip(weights, idxs))
    arr = _SEG_ARRAYS.get(key)
    if arr is None:
        segs, col = [dense_segment(dense, ndense, 0)], ndense
        for w, i in zip(weights, idxs):
            segs.append(table_segment(w, i, col))
            col += w.shape[1]
        arr = _seg_array(segs)
        if len(_SEG_ARRAYS) >= 512:
            _SEG_ARRAYS.clear()
        _SEG_ARRAYS[key] = arr
    return arr


def concat_gather(segs, batch: int, out: torch.Tensor):
    lib = _lib.load()
    _lib.ensure_device(out.device)
    arr = _seg_array(segs)
    check(lib.rk_concat_gather(arr, len(segs), batch, ptr(out), out.stride(0), _lib.stream_of(out)),
          "rk_concat_gather")
    return out


def dcn_cross(segs, batch, width, cross_w, cross_b, num_layers, head_w_ptr, x0, partial, device,
              xl_in=None, xl_out=None):
    lib = _lib.load()
    _lib.ensure_device(device)
    arr = _as_seg_array(segs)
    check(lib.rk_dcn_cross(arr, len(segs), batch, width, ptr(cross_w), ptr(cross_b), num_layers, head_w_ptr,
                           ptr(x0), x0.stride(0) if x0 is not None else 0,
                           ptr(xl_in), xl_in.stride(0) if xl_in is not None else 0,
                           ptr(xl_out), xl_out.stride(0) if xl_out is not None else 0,
                           ptr(partial), _lib.raw_stream(device)), "rk_dcn_cross")


DCN_CROSS_W_SLOT, DCN_CROSS_B_SLOT = 4, 5


def dcn_forward_args(segs, batch, width, cross_w, cross_b, num_layers, cross_head_w, layers, head: Epilogue,
                     device):
    """The rk_dcn_forward argument list (gather + cross stack + MLP tail + head in one launch; the
    stream last, None) — cross_w / cross_b at DCN_CROSS_W_SLOT / DCN_CROSS_B_SLOT are per-call slots."""
    _lib.ensure_device(device)
    arr = _seg_array(segs)
    mls = (_lib.MlpLayer * max(1, len(layers)))(*layers)
    return [arr, len(segs), batch, width, ptr(cross_w), ptr(cross_b), num_layers, cross_head_w.data_ptr(), mls,
            len(layers), ctypes.byref(head), None]


def fm_gather(second, first, dim, batch, deep_in, fm1, fm2):
    lib = _lib.load()
    _lib.ensure_device(deep_in.device)
    a2, a1 = _as_seg_array(second), _as_seg_array(first)
    check(lib.rk_fm_gather(a2, a1, len(second), dim, batch, ptr(deep_in), deep_in.stride(0), ptr(fm1), ptr(fm2),
                           _lib.stream_of(deep_in)), "rk_fm_gather")


def fm_pack_table(second: torch.Tensor, first: torch.Tensor, row_stride: int) -> torch.Tensor:
    """rk_fm_pack_table: [V, D] + [V, 1] -> one [V, row_stride] table (row, then the weight at D)."""
    lib = _lib.load()
    _lib.ensure_device(second.device)
    V, D = second.shape
    if first.shape[0] != V or second.stride(1) != 1:
        raise ValueError("rankops.fm_pack_table: tables of one field must have the same rows")
    out = torch.empty(V, row_stride, device=second.device, dtype=torch.float32)
    check(lib.rk_fm_pack_table(ptr(second), second.stride(0), ptr(first), first.stride(0), V, D, ptr(out),
                               row_stride, _lib.stream_of(out)), "rk_fm_pack_table")
    return out


def fm_gather_packed(fields, dim, batch, deep_in, fm1, fm2):
    """rk_fm_gather_packed: fields = table_segment(packed table, idx, out_col) per field."""
    lib = _lib.load()
    _lib.ensure_device(deep_in.device)
    arr = _seg_array(fields)
    check(lib.rk_fm_gather_packed(arr, len(fields), dim, batch, ptr(deep_in), deep_in.stride(0), ptr(fm1),
                                  ptr(fm2), _lib.stream_of(deep_in)), "rk_fm_gather_packed")


def fm_linear_packed(fields, dim, batch, layer: "_lib.MlpLayer", y, fm1, fm2):
    """rk_fm_linear_packed: the packed FM gather, fm1, fm2 and the first deep layer into y [batch, n]
    in one launch; fields = packed_segment(table, idx, dim, f * dim) per field."""
    lib = _lib.load()
    _lib.ensure_device(y.device)
    arr = _seg_array(fields)
    check(lib.rk_fm_linear_packed(arr, len(fields), dim, batch, ctypes.byref(layer), ptr(y), y.stride(0), ptr(fm1),
                                  ptr(fm2), _lib.stream_of(y)), "rk_fm_linear_packed")


# (fm1, fm2) argument slots of the launch that opens a DeepFM eval forward, by entry point
FM_OUT_SLOTS = {"rk_fm_gather_packed": (6, 7), "rk_fm_linear_packed": (7, 8), "rk_deepfm_forward": (7, 8)}


def deepfm_whole_plan(k0: int, widths) -> bool:
    """Whether rk_deepfm_forward has a compiled plan for this DeepFM (deep input k0 wide, hidden
    widths): 960 -> 512 -> 256 -> 128 (configs[1]); RANKOPS_MLP_STREAM=0 turns it off, as in C."""
    return (os.environ.get("RANKOPS_MLP_STREAM", "1")[:1] != "0" and (k0 + 63) // 64 * 64 == 960
            and list(widths) == [512, 256, 128])


def deepfm_forward(fields, dim, batch, layers, ep, fm1, fm2):
    """rk_deepfm_forward: the whole DeepFM eval forward in one launch (packed gather, FM, the deep
    layers and the head); fields = packed_segment(table, idx, dim, f * dim) per field, layers the
    three MlpLayer structs, ep the head epilogue (head_w/b, final_w/b, head_logit/prob/aux)."""
    lib = _lib.load()
    _lib.ensure_device(fm1.device)
    arr = _seg_array(fields)
    la = (_lib.MlpLayer * len(layers))(*layers)
    check(lib.rk_deepfm_forward(arr, len(fields), dim, batch, la, len(layers), ctypes.byref(ep), ptr(fm1), ptr(fm2),
                                _lib.stream_of(fm1)), "rk_deepfm_forward")


def deepfm_forward_fo(fields, first, first_ld, dim, batch, layers, ep, fm1, fm2):
    """rk_deepfm_forward_fo: rk_deepfm_forward with the first-order weights from their own sources
    (first[f]: a device address or None, first_ld[f] its row stride in floats)."""
    lib = _lib.load()
    _lib.ensure_device(fm1.device)
    arr = _seg_array(fields)
    n = len(fields)
    fp = (ctypes.c_void_p * n)(*[x or None for x in first])
    fl = (ctypes.c_int64 * n)(*first_ld)
    la = (_lib.MlpLayer * len(layers))(*layers)
    check(lib.rk_deepfm_forward_fo(arr, fp, fl, n, dim, batch, la, len(layers), ctypes.byref(ep), ptr(fm1), ptr(fm2),
                                   _lib.stream_of(fm1)), "rk_deepfm_forward_fo")


CIN_ACT = {"identity": _lib.RK_ACT_NONE, "relu": _lib.RK_ACT_RELU}


def pack_cin_weight(weight: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """One CIN layer's weight ([n, k], or nn.Conv1d's [n, k, 1]) -> rk_cin_pack_weight's image, a flat
    pad16(n) * pad16(k) tensor (into `out` when given: a previous image of the same shape)."""
    lib = _lib.load()
    require_gpu(weight, "cin weight")
    if weight.dtype != torch.float32 or weight.dim() not in (2, 3) or (weight.dim() == 3 and weight.shape[2] != 1):
        raise ValueError(f"pack_cin_weight: expected a float32 [n, k] or [n, k, 1] weight, got {tuple(weight.shape)}")
    n, k = weight.shape[0], weight.shape[1]
    w = weight.detach().reshape(n, k)
    if w.stride(1) != 1:
        w = w.contiguous()
    size = (n + 15) // 16 * 16 * ((k + 15) // 16 * 16)
    if out is None or out.numel() != size or out.device != w.device:
        out = torch.empty(size, device=w.device, dtype=torch.float32)
    check(lib.rk_cin_pack_weight(w.data_ptr(), w.stride(0), n, k, out.data_ptr(), _lib.stream_of(out)),
          "rk_cin_pack_weight")
    return out


def cin_forward_args(second, first, dim, batch, images, biases, sizes, activation, out_w, out_b, deep_in, fm1, pooled,
                     cin_logit, device):
    """The rk_cin_forward argument list (the stream last, None) and the ctypes arrays it points into.
    fm1 at [14], cin_logit at [17] and the stream at [-1] are the per-call slots of a cached forward."""
    _lib.ensure_device(device)
    nl = len(images)
    a2 = _as_seg_array(second)
    a1 = _as_seg_array(first) if first is not None else None
    wp = (ctypes.c_void_p * max(1, nl))(*[ptr(w) for w in images])
    bp = (ctypes.c_void_p * max(1, nl))(*[ptr(b) for b in biases])
    hs = (ctypes.c_int32 * max(1, nl))(*[int(h) for h in sizes])
    act = CIN_ACT[activation] if isinstance(activation, str) else int(activation)
    args = [a2, a1, len(second), dim, batch, wp, bp, hs, nl, act, ptr(out_w), ptr(out_b), ptr(deep_in),
            deep_in.stride(0) if deep_in is not None else 0, ptr(fm1), ptr(pooled),
            pooled.stride(0) if pooled is not None else 0, ptr(cin_logit), None]
    return args, (a2, a1, wp, bp, hs)


def cin_forward(second, first, dim, batch, images, biases, sizes, activation, device, *, out_w=None, out_b=None,
                deep_in=None, fm1=None, pooled=None, cin_logit=None):
    """rk_cin_forward: row gather, first-order sum, every CIN layer, the pooling over d and the output
    layer in one launch.  second / first: lists of Segments (all tables or all dense; first may be
    None without fm1), images: pack_cin_weight() of each layer, sizes: H_k; every output is optional."""
    args, _keep = cin_forward_args(second, first, dim, batch, images, biases, sizes, activation, out_w, out_b,
                                   deep_in, fm1, pooled, cin_logit, device)
    args[-1] = _lib.raw_stream(device)
    check(_lib.load().rk_cin_forward(*args), "rk_cin_forward")


FIBINET_TYPES = {"all": 0, "each": 1, "interaction": 2}  # RK_FIBINET_ALL / EACH / INTERACTION
# argument slots of the two FiBiNET launches patched per call
FIBINET_LINEAR_SLOT = 13                   # rk_fibinet_interaction: linear
FIBINET_OUT_SLOTS = (20, 19, 17, 18)       # rk_fibinet_forward: prob, total_logit, linear, deep_logit


def fibinet_matrices(num_fields: int, bilinear_type: str) -> int:
    """How many D x D matrices each bilinear layer of this type holds."""
    if bilinear_type not in FIBINET_TYPES:
        raise ValueError(f"bilinear_type must be one of {sorted(FIBINET_TYPES)}, got {bilinear_type!r}")
    m = int(num_fields)
    return {"all": 1, "each": m - 1, "interaction": m * (m - 1) // 2}[bilinear_type]


def _fibinet_front(second, first, dim, batch, senet_w1, senet_w2, bilinear_e, bilinear_v, bilinear_type, device):
    _lib.ensure_device(device)
    a2 = _as_seg_array(second)
    a1 = _as_seg_array(first) if first is not None else None
    return [a2, a1, len(second), dim, batch, ptr(senet_w1), ptr(senet_w2), senet_w1.shape[0], ptr(bilinear_e),
            ptr(bilinear_v), FIBINET_TYPES[bilinear_type]], (a2, a1)


def fibinet_interaction_args(second, first, dim, batch, senet_w1, senet_w2, bilinear_e, bilinear_v, bilinear_type, c,
                             linear, attention, device):
    """The rk_fibinet_interaction argument list (the stream last, None) and the ctypes arrays it points
    into.  senet_w1 [r, m] / senet_w2 [m, r] contiguous, bilinear_e / bilinear_v the stacked contiguous
    [nmat, D, D] weights; linear at [FIBINET_LINEAR_SLOT] is the per-call slot of a cached forward."""
    args, keep = _fibinet_front(second, first, dim, batch, senet_w1, senet_w2, bilinear_e, bilinear_v, bilinear_type,
                                device)
    args += [ptr(c), c.stride(0), ptr(linear), ptr(attention), attention.stride(0) if attention is not None else 0,
             None]
    return args, keep


def fibinet_forward_args(second, first, dim, batch, senet_w1, senet_w2, bilinear_e, bilinear_v, bilinear_type, layers,
                         head_w, head_b, final_w, final_b, device):
    """The rk_fibinet_forward argument list (the stream last, None; the four outputs at FIBINET_OUT_SLOTS
    are per-call slots) and the ctypes arrays it points into.  layers: MlpLayer structs over packed images."""
    args, keep = _fibinet_front(second, first, dim, batch, senet_w1, senet_w2, bilinear_e, bilinear_v, bilinear_type,
                                device)
    la = (_lib.MlpLayer * max(1, len(layers)))(*layers)
    args += [la, len(layers), ptr(head_w), ptr(head_b), ptr(final_w), ptr(final_b), None, None, None, None, None]
    return args, keep + (la,)


def fibinet_interaction(x0: torch.Tensor, senet_w1: torch.Tensor, senet_w2: torch.Tensor, bilinear_e, bilinear_v,
                        bilinear_type: str = "interaction", return_attention: bool = False):
    """FiBiNET's SENET field attention and bilinear interaction over dense rows x0 [B, m, D] (any row
    stride; field rows 16-B aligned), one launch (rk_fibinet_interaction):

        z[b, i] = mean_d x0[b, i, d],  a[b, :] = relu(senet_w2 relu(senet_w1 z[b, :])),  v = a[..., None] * x0
        p[b, (i, j), :] = (We x0[b, i, :]) * x0[b, j, :],  q[b, (i, j), :] = (Wv v[b, i, :]) * v[b, j, :]

    over the pairs i < j in lexicographic order, W x = nn.Linear's x @ W.T.  senet_w1 [r, m], senet_w2
    [m, r]; bilinear_e / bilinear_v: lists of [D, D] weights, 1 ("all"), m - 1 ("each": We = the left
    field's) or m (m - 1) / 2 ("interaction": the pair's) of them.  Returns c [B, m (m - 1) D] = all of
    p, then all of q; with return_attention=True also a [B, m]."""
    as_f32(x0, "x0")
    if x0.dim() != 3 or x0.stride(2) != 1:
        raise ValueError(f"rankops.fibinet_interaction: x0 must be [B, m, D] with unit stride along D, got "
                         f"{tuple(x0.shape)}")
    B, m, D = x0.shape
    nmat = fibinet_matrices(m, bilinear_type)
    bilinear_e, bilinear_v = list(bilinear_e), list(bilinear_v)
    for name, ws in (("bilinear_e", bilinear_e), ("bilinear_v", bilinear_v)):
        if len(ws) != nmat or any(tuple(as_f32(w, name).shape) != (D, D) for w in ws):
            raise ValueError(f"rankops.fibinet_interaction: {name} must be {nmat} weights of shape {(D, D)} for "
                             f"bilinear_type {bilinear_type!r}")
    as_f32(senet_w1, "senet_w1"), as_f32(senet_w2, "senet_w2")
    r = senet_w1.shape[0]
    if senet_w1.dim() != 2 or tuple(senet_w1.shape) != (r, m) or tuple(senet_w2.shape) != (m, r):
        raise ValueError(f"rankops.fibinet_interaction: senet_w1 must be [r, {m}] and senet_w2 [{m}, r], got "
                         f"{tuple(senet_w1.shape)} and {tuple(senet_w2.shape)}")
    dev = x0.device
    c = torch.empty(B, m * (m - 1) * D, device=dev, dtype=torch.float32)
    attn = torch.empty(B, m, device=dev, dtype=torch.float32) if return_attention else None
    if B > 0:
        be = torch.stack([w.detach() for w in bilinear_e]).contiguous()
        bv = torch.stack([w.detach() for w in bilinear_v]).contiguous()
        w1, w2 = senet_w1.detach().contiguous(), senet_w2.detach().contiguous()
        segs = [Segment(fptr(x0, i * x0.stride(1)), None, 0, x0.stride(0), 0, D, i * D) for i in range(m)]
        args, _keep = fibinet_interaction_args(segs, None, D, B, w1, w2, be, bv, bilinear_type, c, None, attn, dev)
        args[-1] = _lib.raw_stream(dev)
        check(_lib.load().rk_fibinet_interaction(*args), "rk_fibinet_interaction")
    return (c, attn) if return_attention else c


def pack_cin_weight_t(weight: torch.Tensor, num_fields: int, out: torch.Tensor = None) -> torch.Tensor:
    """One CIN layer's weight ([n, hprev * num_fields] or nn.Conv1d's [n, k, 1]) -> rk_cin_pack_weight_t's
    image for rk_cin_backward: W^T, field-major, a flat num_fields * pad16(hprev) * pad16(n) tensor
    (into `out` when given: a previous image of the same shape)."""
    lib = _lib.load()
    require_gpu(weight, "cin weight")
    if weight.dtype != torch.float32 or weight.dim() not in (2, 3) or (weight.dim() == 3 and weight.shape[2] != 1):
        raise ValueError(f"pack_cin_weight_t: expected a float32 [n, k] or [n, k, 1] weight, got {tuple(weight.shape)}")
    n, k = weight.shape[0], weight.shape[1]
    if num_fields <= 0 or k % num_fields:
        raise ValueError(f"pack_cin_weight_t: {k} columns are no multiple of {num_fields} fields")
    w = weight.detach().reshape(n, k)
    if w.stride(1) != 1:
        w = w.contiguous()
    hprev = k // num_fields
    size = num_fields * ((hprev + 15) // 16 * 16) * ((n + 15) // 16 * 16)
    if out is None or out.numel() != size or out.device != w.device:
        out = torch.empty(size, device=w.device, dtype=torch.float32)
    check(lib.rk_cin_pack_weight_t(w.data_ptr(), w.stride(0), n, hprev, num_fields, out.data_ptr(),
                                   _lib.stream_of(out)), "rk_cin_pack_weight_t")
    return out


def cin_forward_train(second, first, dim, batch, images, biases, sizes, activation, device, maps, *, out_w=None,
                      out_b=None, deep_in=None, fm1=None, pooled=None, cin_logit=None):
    """rk_cin_forward_train: cin_forward that also writes every layer's feature maps into
    maps [batch, sum H_k, dim] (contiguous) for cin_backward / cin_wgrad."""
    args, _keep = cin_forward_args(second, first, dim, batch, images, biases, sizes, activation, out_w, out_b,
                                   deep_in, fm1, pooled, cin_logit, device)
    if maps.shape != (batch, sum(int(h) for h in sizes), dim) or not maps.is_contiguous():
        raise ValueError(f"cin_forward_train: maps must be contiguous [batch, sum H_k, dim], got {tuple(maps.shape)}")
    args[-1:] = [maps.data_ptr(), _lib.raw_stream(device)]
    check(_lib.load().rk_cin_forward_train(*args), "rk_cin_forward_train")


def _rows_ok(t):
    return t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0


def cin_backward(x0_rows, num_fields, dim, images_t, sizes, activation, maps, *, dpooled=None, dlogit=None,
                 out_w=None, dx0_add=None, dx0=None, dy=None):
    """rk_cin_backward: the CIN's data backward in one launch.  x0_rows [B, >= m D] (field i at column
    i D; 16-B aligned rows), images_t: pack_cin_weight_t() of each layer, maps: cin_forward_train's.
    The gradient of pooled is dpooled [B, sum H_k] and / or dlogit [B] * out_w.  Returns
    (dx0 [B, m D] (+ dx0_add), dy [B, sum H_k, D]: the pre-activation gradients cin_wgrad reads)."""
    B, dev = x0_rows.shape[0], x0_rows.device
    _lib.ensure_device(dev)
    nl = len(images_t)
    if dx0 is None:
        dx0 = torch.empty(B, num_fields * dim, device=dev, dtype=torch.float32)
    if dy is None:
        dy = torch.empty_like(maps)
    for t, what in ((x0_rows, "x0_rows"), (dx0, "dx0"), (dx0_add, "dx0_add")):
        if t is not None and B > 0 and not _rows_ok(t):
            raise ValueError(f"cin_backward: {what} needs unit column stride and 16-B aligned rows")
    if dpooled is not None and dpooled.stride(1) != 1:
        dpooled = dpooled.contiguous()
    wp = (ctypes.c_void_p * max(1, nl))(*[ptr(w) for w in images_t])
    hs = (ctypes.c_int32 * max(1, nl))(*[int(h) for h in sizes])
    act = CIN_ACT[activation] if isinstance(activation, str) else int(activation)
    check(_lib.load().rk_cin_backward(
        ptr(x0_rows), x0_rows.stride(0), num_fields, dim, B, wp, hs, nl, act, ptr(maps), ptr(dpooled),
        dpooled.stride(0) if dpooled is not None else 0, ptr(dlogit), ptr(out_w), ptr(dx0_add),
        dx0_add.stride(0) if dx0_add is not None else 0, ptr(dx0), dx0.stride(0), ptr(dy), _lib.raw_stream(dev)),
        "rk_cin_backward")
    return dx0, dy


def cin_wgrad_workspace(num_fields, sizes, device):
    nl = len(sizes)
    hs = (ctypes.c_int32 * max(1, nl))(*[int(h) for h in sizes])
    n = _lib.load().rk_cin_wgrad_workspace_floats(num_fields, hs, nl)
    return torch.empty(max(1, n), device=device, dtype=torch.float32)


def cin_wgrad(x0_rows, num_fields, dim, sizes, maps, dy, *, bias=True, workspace=None):
    """rk_cin_wgrad: ([dW_k [H_k, H_{k-1} m]], [dbias_k [H_k]] or None) of every layer from the rows,
    the saved maps and cin_backward's dy; slabs of the reduction are added in a fixed order."""
    B, dev = x0_rows.shape[0], x0_rows.device
    _lib.ensure_device(dev)
    nl = len(sizes)
    if B > 0 and not _rows_ok(x0_rows):
        raise ValueError("cin_wgrad: x0_rows needs unit column stride and 16-B aligned rows")
    dws, dbs, hprev = [], [], num_fields
    for h in sizes:
        dws.append(torch.empty(int(h), hprev * num_fields, device=dev, dtype=torch.float32))
        dbs.append(torch.empty(int(h), device=dev, dtype=torch.float32) if bias else None)
        hprev = int(h)
    if workspace is None:
        workspace = cin_wgrad_workspace(num_fields, sizes, dev)
    hs = (ctypes.c_int32 * max(1, nl))(*[int(h) for h in sizes])
    wp = (ctypes.c_void_p * max(1, nl))(*[ptr(w) for w in dws])
    bp = (ctypes.c_void_p * max(1, nl))(*[ptr(b) for b in dbs])
    check(_lib.load().rk_cin_wgrad(ptr(x0_rows), x0_rows.stride(0), num_fields, dim, B, hs, nl, ptr(maps), ptr(dy),
                                   wp, bp, workspace.data_ptr(), workspace.numel(), _lib.raw_stream(dev)),
          "rk_cin_wgrad")
    return dws, (dbs if bias else None)


def _cin_launch(x0, weights, biases, sizes, activation, out_w, out_b, maps):
    """pooled (and the logit with out_w) of rankops.cin's rows; with `maps` through rk_cin_forward_train."""
    B, m, D = x0.shape
    dev = x0.device
    pooled = torch.empty(B, sum(sizes), device=dev, dtype=torch.float32)
    logit = torch.empty(B, 1, device=dev, dtype=torch.float32) if out_w is not None else None
    if B > 0:
        images = [pack_cin_weight(w) for w in weights]
        biases = [b if b is None or b.is_contiguous() else b.contiguous() for b in biases]
        segs = [Segment(fptr(x0, i * x0.stride(1)), None, 0, x0.stride(0), 0, D, i * D) for i in range(m)]
        if maps is None:
            cin_forward(segs, None, D, B, images, biases, sizes, activation, dev, out_w=out_w, out_b=out_b,
                        pooled=pooled, cin_logit=logit)
        else:
            cin_forward_train(segs, None, D, B, images, biases, sizes, activation, dev, maps, out_w=out_w,
                              out_b=out_b, pooled=pooled, cin_logit=logit)
    return pooled, logit


class _CinFn(torch.autograd.Function):
    """rankops.cin under autograd: rk_cin_forward_train, then rk_cin_backward + rk_cin_wgrad (and
    rk_logit_head_backward for the output layer).  Inputs: x0, out_w, out_b, the weights, the biases."""

    @staticmethod
    def forward(ctx, activation, nl, x0, out_w, out_b, *wb):
        weights, biases = list(wb[:nl]), list(wb[nl:])
        B, m, D = x0.shape
        sizes = [w.shape[0] for w in weights]
        x0, out_w, out_b = x0.detach(), _detach(out_w), _detach(out_b)
        maps = torch.empty(B, sum(sizes), D, device=x0.device, dtype=torch.float32)
        pooled, logit = _cin_launch(x0, [w.detach() for w in weights], [_detach(b) for b in biases], sizes,
                                    activation, out_w, out_b, maps)
        ctx.activation, ctx.nl, ctx.sizes, ctx.shape = activation, nl, sizes, (B, m, D)
        ctx.save_for_backward(x0, maps, pooled, out_w, *weights)
        ctx.mark_non_differentiable(maps)
        if logit is None:
            return pooled, maps
        return pooled, logit, maps

    @staticmethod
    def backward(ctx, dpooled, *rest):
        x0, maps, pooled, out_w, *weights = ctx.saved_tensors
        dlogit = rest[0] if len(rest) == 2 else None
        B, m, D = ctx.shape
        nl, sizes, dev = ctx.nl, ctx.sizes, x0.device
        need = ctx.needs_input_grad  # (activation, nl, x0, out_w, out_b, weights.., biases..)
        if dpooled is None and dlogit is None:
            return (None,) * (5 + 2 * nl)
        if B == 0:  # nothing to launch: zero gradients of every shape
            zero = lambda t, n: torch.zeros_like(t) if n and t is not None else None  # noqa: E731
            return (None, None, *[zero(t, n) for t, n in zip((x0, out_w), need[2:4])],
                    torch.zeros(1, device=dev) if need[4] else None,
                    *[zero(w, n) for w, n in zip(weights, need[5:5 + nl])],
                    *[torch.zeros(h, device=dev) if n else None for h, n in zip(sizes, need[5 + nl:])])
        if dpooled is not None:
            dpooled = dpooled.to(torch.float32)
        dl = dlogit.to(torch.float32).reshape(B).contiguous() if dlogit is not None else None
        d_out_w = d_out_b = None
        if dl is not None and (need[3] or need[4]):
            d_out_w = torch.empty(1, sum(sizes), device=dev, dtype=torch.float32)
            d_out_b = torch.empty(1, device=dev, dtype=torch.float32)
            logit_head_backward(dl, None, None, pooled, None, out_w, None, None, d_out_w, d_out_b)
        elif need[3] or need[4]:
            d_out_w = torch.zeros(1, sum(sizes), device=dev, dtype=torch.float32)
            d_out_b = torch.zeros(1, device=dev, dtype=torch.float32)
        if B > 0 and x0.stride(1) == D and x0.stride(0) % 4 == 0 and x0.data_ptr() % 16 == 0 and (
                B == 1 or x0.stride(0) >= m * D):
            rows = x0.as_strided((B, m * D), (x0.stride(0), 1))  # the caller's rows, whatever their stride
        else:
            rows = x0.contiguous().view(B, m * D)
        images_t = [pack_cin_weight_t(w, m) for w in weights]
        dx0, dy = cin_backward(rows, m, D, images_t, sizes, ctx.activation, maps, dpooled=dpooled, dlogit=dl,
                               out_w=out_w if dl is not None else None)
        dws = dbs = [None] * nl
        if any(need[5:]):
            dws, dbs = cin_wgrad(rows, m, D, sizes, maps, dy)
            dws = [g.view(w.shape) for g, w in zip(dws, weights)]
        return (None, None, dx0.view(B, m, D) if need[2] else None,
                d_out_w.view(out_w.shape) if need[3] else None, d_out_b if need[4] else None,
                *[g if n else None for g, n in zip(dws, need[5:5 + nl])],
                *[g if n else None for g, n in zip(dbs, need[5 + nl:])])


def _detach(t):
    return None if t is None else t.detach()


def cin(x0: torch.Tensor, weights, biases=None, activation: str = "identity", out_w=None, out_b=None,
        return_maps: bool = False):
    """The Compressed Interaction Network over dense rows x0 [B, m, D] (any row stride; field rows
    16-B aligned): x^k[b, n, d] = act(sum_{h, i} W_k[n, h m + i] x^{k-1}[b, h, d] x0[b, i, d] + bias_k[n])
    for weights[k] of shape [H_k, H_{k-1} m] (or nn.Conv1d's [H_k, H_{k-1} m, 1]), H_0 = m.  Returns
    pooled [B, sum H_k] (the sums over d, layers side by side); with out_w [sum H_k] and out_b [1]
    also the logit pooled . out_w + out_b as (pooled, logit [B, 1]).

    Differentiable: with grad enabled and x0, a weight, a bias, out_w or out_b requiring grad the call
    goes through autograd (HIP backward: rk_cin_backward, rk_cin_wgrad); with plain tensors it is the
    eval launch.  return_maps=True appends the list of feature maps x^k as [B, H_k, D] views (no
    gradient flows through them)."""
    as_f32(x0, "x0")
    if activation not in CIN_ACT:
        raise ValueError(f"rankops.cin: activation must be one of {sorted(CIN_ACT)}, got {activation!r}")
    if x0.dim() != 3 or x0.stride(2) != 1:
        raise ValueError(f"rankops.cin: x0 must be [B, m, D] with unit stride along D, got {tuple(x0.shape)}")
    B, m, D = x0.shape
    weights = list(weights)
    biases = list(biases) if biases is not None else [None] * len(weights)
    sizes, hprev = [], m
    for k, w in enumerate(weights):
        as_f32(w, f"weights[{k}]")
        if w.shape[1] != hprev * m:
            raise ValueError(f"rankops.cin: weights[{k}] has {w.shape[1]} columns, expected {hprev * m}")
        if biases[k] is not None and as_f32(biases[k], f"biases[{k}]").numel() != w.shape[0]:
            raise ValueError(f"rankops.cin: biases[{k}] must have {w.shape[0]} elements")
        hprev = w.shape[0]
        sizes.append(hprev)
    grad = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (x0, out_w, out_b, *weights, *biases))
    if grad:
        *out, maps = _CinFn.apply(activation, len(weights), x0, out_w, out_b, *weights, *biases)
    else:
        maps = torch.empty(B, sum(sizes), D, device=x0.device, dtype=torch.float32) if return_maps else None
        pooled, logit = _cin_launch(x0, weights, biases, sizes, activation, out_w, out_b, maps)
        out = [pooled] if out_w is None else [pooled, logit]
    if return_maps:
        offs = [sum(sizes[:k]) for k in range(len(sizes))]
        out.append([maps[:, o:o + h] for o, h in zip(offs, sizes)])
    return out[0] if len(out) == 1 else tuple(out)


def din_attention(query_ptr, ld_query, key_table, seq, seq_len, T, H, weights, use_softmax, out_ptr, ld_out,
                  batch, device):
    lib = _lib.load()
    _lib.ensure_device(device)
    w1, b1, w2, b2, w3, b3 = weights
    check(lib.rk_din_attention(query_ptr, ld_query, ptr(key_table), key_table.shape[0], key_table.stride(0),
                               ptr(seq), seq.stride(0), T, ptr(seq_len), batch, H, ptr(w1), ptr(b1), ptr(w2),
                               ptr(b2), ptr(w3), ptr(b3), 1 if use_softmax else 0, out_ptr, ld_out,
                               _lib.raw_stream(device)), "rk_din_attention")


def din_attention_dense(query, keys, keys_length, weights, use_softmax, out):
    """rk_din_attention_dense: keys [B, T, H] (rows 16-B aligned), query/out [B, H]."""
    lib = _lib.load()
    _lib.ensure_device(keys.device)
    w1, b1, w2, b2, w3, b3 = weights
    B, T, H = keys.shape
    check(lib.rk_din_attention_dense(ptr(query), query.stride(0), ptr(keys), keys.stride(0), keys.stride(1), T,
                                     ptr(keys_length), B, H, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3),
                                     1 if use_softmax else 0, ptr(out), out.stride(0), _lib.stream_of(keys)),
          "rk_din_attention_dense")


DIEN_CELLS = {"AGRU": 0, "AUGRU": 1}


def dien_interest(query_ptr, ld_query, key_table, seq, seq_len, T, H, nh, cell_type, weights, out_ptr, ld_out,
                  att, batch, device):
    """rk_dien_interest: GRU + attention + AGRU/AUGRU over key_table[seq] in one launch; query / out
    are strided pointers (they may lie in one row buffer), weights = (Wg, bg, Wc, bc, A, Vg, vg, Vc,
    vc), att an optional [batch, T] output of the attention weights."""
    lib = _lib.load()
    _lib.ensure_device(device)
    check(lib.rk_dien_interest(query_ptr, ld_query, ptr(key_table), key_table.shape[0], key_table.stride(0),
                               ptr(seq), seq.stride(0), T, ptr(seq_len), batch, H, nh, cell_type,
                               *[ptr(w) for w in weights], out_ptr, ld_out, ptr(att),
                               att.stride(0) if att is not None else 0, _lib.raw_stream(device)),
          "rk_dien_interest")


def dien_interest_dense(query, keys, keys_length, nh, cell_type, weights, out, att):
    """rk_dien_interest_dense: keys [B, T, H] (rows 16-B aligned), query [B, H], out [B, nh]."""
    lib = _lib.load()
    _lib.ensure_device(keys.device)
    B, T, H = keys.shape
    check(lib.rk_dien_interest_dense(ptr(query), query.stride(0), ptr(keys), keys.stride(0), keys.stride(1), T,
                                     ptr(keys_length), B, H, nh, cell_type, *[ptr(w) for w in weights], ptr(out),
                                     out.stride(0), ptr(att), att.stride(0) if att is not None else 0,
                                     _lib.stream_of(keys)), "rk_dien_interest_dense")


def dien_interest_train(query_ptr, ld_query, key_table, seq, seq_len, T, H, nh, cell_type, weights, out_ptr, ld_out,
                        att, hs, ss, batch, device):
    """rk_dien_interest_train: rk_dien_interest that also keeps the extractor states hs [batch, T, nh],
    the evolution states ss [batch, T, nh] and the attention weights att [batch, T] for the backward."""
    lib = _lib.load()
    _lib.ensure_device(device)
    check(lib.rk_dien_interest_train(query_ptr, ld_query, ptr(key_table), key_table.shape[0], key_table.stride(0),
                                     ptr(seq), seq.stride(0), T, ptr(seq_len), batch, H, nh, cell_type,
                                     *[ptr(w) for w in weights], out_ptr, ld_out, ptr(att), att.stride(0), ptr(hs),
                                     ptr(ss), _lib.raw_stream(device)), "rk_dien_interest_train")


def dien_interest_train_dense(query, keys, keys_length, nh, cell_type, weights, out, att, hs, ss):
    """rk_dien_interest_train_dense: the same over keys [B, T, H] (rows 16-B aligned)."""
    lib = _lib.load()
    _lib.ensure_device(keys.device)
    B, T, H = keys.shape
    check(lib.rk_dien_interest_train_dense(ptr(query), query.stride(0), ptr(keys), keys.stride(0), keys.stride(1), T,
                                           ptr(keys_length), B, H, nh, cell_type, *[ptr(w) for w in weights],
                                           ptr(out), out.stride(0), ptr(att), att.stride(0), ptr(hs), ptr(ss),
                                           _lib.stream_of(keys)), "rk_dien_interest_train_dense")


def dien_extract(key_table, seq, seq_len, T, H, nh, weights, hs, requests, device):
    """rk_dien_extract: the interest extractor over key_table[seq] once per request -> hs [requests, T, nh]
    (rows t >= seq_len zero); weights = (Wg, bg, Wc, bc)."""
    lib = _lib.load()
    _lib.ensure_device(device)
    check(lib.rk_dien_extract(ptr(key_table), key_table.shape[0], key_table.stride(0), ptr(seq), seq.stride(0), T,
                              ptr(seq_len), requests, H, nh, *[ptr(w) for w in weights], ptr(hs),
                              _lib.raw_stream(device)), "rk_dien_extract")


def dien_extract_dense(keys, keys_length, nh, weights, hs):
    """rk_dien_extract_dense: the same over keys [R, T, H] (rows 16-B aligned)."""
    lib = _lib.load()
    _lib.ensure_device(keys.device)
    R, T, H = keys.shape
    check(lib.rk_dien_extract_dense(ptr(keys), keys.stride(0), keys.stride(1), T, ptr(keys_length), R, H, nh,
                                    *[ptr(w) for w in weights], ptr(hs), _lib.stream_of(keys)),
          "rk_dien_extract_dense")


def dien_evolve(query_ptr, ld_query, hs, seq_len, request_index, H, cell_type, weights, out_ptr, ld_out, att, batch,
                device):
    """rk_dien_evolve: attention + AGRU/AUGRU of candidate b over hs[request_index[b]] (hs [R, T, nh]
    contiguous); query / out are strided pointers (they may lie in one row buffer), weights =
    (A, Vg, vg, Vc, vc), att an optional [batch, T] output of the attention weights."""
    lib = _lib.load()
    _lib.ensure_device(device)
    R, T, nh = hs.shape
    check(lib.rk_dien_evolve(query_ptr, ld_query, ptr(hs), R, T, ptr(seq_len), ptr(request_index), batch, H, nh,
                             cell_type, *[ptr(w) for w in weights], out_ptr, ld_out, ptr(att),
                             att.stride(0) if att is not None else 0, _lib.raw_stream(device)), "rk_dien_evolve")


def _dien_forward_args(segs, width, q_col, state_col, key_table, seq, seq_len, H, nh, cell_type, weights, layers,
                       head: Epilogue, att, batch):
    """The rk_dien_forward argument list (without the stream / plan slot) and the ctypes arrays it
    points into."""
    arr = _seg_array(segs)
    larr = (_lib.MlpLayer * max(1, len(layers)))(*layers)
    args = (arr, len(segs), width, q_col, state_col, ptr(key_table), key_table.shape[0], key_table.stride(0), ptr(seq),
            seq.stride(0), seq.shape[1], ptr(seq_len), batch, H, nh, cell_type, *[ptr(w) for w in weights], larr,
            len(layers), ctypes.byref(head), ptr(att), att.stride(0) if att is not None else 0)
    return args, (arr, larr, head)


def dien_forward(segs, width, q_col, state_col, key_table, seq, seq_len, H, nh, cell_type, weights, layers,
                 head: Epilogue, att, batch, device):
    """rk_dien_forward: the whole DIEN eval forward (row gather, GRU + attention + AGRU/AUGRU, fcn tail,
    head) in one launch; weights = (Wg, bg, Wc, bc, A, Vg, vg, Vc, vc), att an optional [batch, T]
    output of the attention weights."""
    lib = _lib.load()
    _lib.ensure_device(device)
    args, _keep = _dien_forward_args(segs, width, q_col, state_col, key_table, seq, seq_len, H, nh, cell_type,
                                     weights, layers, head, att, batch)
    check(lib.rk_dien_forward(*args, _lib.raw_stream(device)), "rk_dien_forward")


class DienPlan:
    """rk_dien_forward_plan: the one-launch DIEN forward with its arguments validated once; launch()
    runs the kernel on the current stream (no per-call host work besides the ctypes call).  Binds
    the pointers it was made with — `keep` holds every tensor it reads or writes alive for the
    plan's lifetime."""

    def __init__(self, args, keep, device):
        self._lib = _lib.load()
        self._device = device
        self._handle = ctypes.c_void_p()
        check(self._lib.rk_dien_forward_plan(*args, ctypes.byref(self._handle)), "rk_dien_forward_plan")
        self._keep = keep

    def launch(self):
        check(self._lib.rk_dien_plan_launch(self._handle, _lib.raw_stream(self._device)), "rk_dien_plan_launch")

    def launch_on(self, stream: int):
        """Launch on an explicit HIP stream (a raw handle, e.g. `torch.cuda.Stream().cuda_stream`),
        without making it the current stream."""
        check(self._lib.rk_dien_plan_launch(self._handle, ctypes.c_void_p(stream)), "rk_dien_plan_launch")

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            self._lib.rk_dien_plan_destroy(h)
            h.value = None


def dien_forward_plan(segs, width, q_col, state_col, key_table, seq, seq_len, H, nh, cell_type, weights, layers,
                      head: Epilogue, att, batch, device, keep=()):
    _lib.ensure_device(device)
    args, k = _dien_forward_args(segs, width, q_col, state_col, key_table, seq, seq_len, H, nh, cell_type, weights,
                                 layers, head, att, batch)
    return DienPlan(args, (k, tuple(keep)), device)


def dien_interest_backward(query_ptr, ld_query, keys, seq, ld_keys_b, seq_len, T, H, nh, cell_type, weights, hs, ss,
                           att, d_out_ptr, ld_dout, dquery_ptr, ld_dquery, accumulate_dquery, dkeys, batch, device,
                           seq_masked=None, d_hs=None, accumulate_dkeys=False):
    """rk_dien_interest_backward: backprop through time of the interest recurrence.  `keys` is the
    table [V, H] with ids `seq` [batch, T], or the dense history [batch, T, H] with seq None and
    ld_keys_b its batch stride; d_out / dquery are strided pointers (they may lie in one row-gradient
    buffer), dquery is added to when accumulate_dquery; dkeys [batch, T, H] is written (rows past the
    length zero); seq_masked [batch, T] int64, when given, receives the ids with 0 past the length
    (what the embedding scatter of dkeys takes).  d_hs [batch, T, nh] (contiguous) or accumulate_dkeys
    send the call to rk_dien_interest_backward_aux: d_hs is an extra dL/dh_t (the auxiliary loss's),
    accumulate_dkeys adds to a dkeys the caller has already written in full.
    Returns the nine weight gradients (Wg, bg, Wc, bc, A, Vg, vg, Vc, vc)."""
    lib = _lib.load()
    _lib.ensure_device(device)
    grads = [torch.empty_like(w) for w in weights]
    nws = lib.rk_dien_interest_backward_workspace_floats(batch, T, H, nh)
    ws = torch.empty(max(nws, 1), device=device, dtype=torch.float32)
    dense = seq is None
    head = (query_ptr, ld_query, ptr(keys), 0 if dense else keys.shape[0], keys.stride(1) if dense else keys.stride(0),
            ptr(seq), 0 if dense else seq.stride(0), ld_keys_b, T, ptr(seq_len), batch, H, nh, cell_type,
            *[ptr(w) for w in weights], ptr(hs), ptr(ss), ptr(att), att.stride(0), d_out_ptr, ld_dout, dquery_ptr,
            ld_dquery, int(accumulate_dquery), ptr(dkeys), *[ptr(g) for g in grads], ptr(seq_masked))
    if d_hs is None and not accumulate_dkeys:
        check(lib.rk_dien_interest_backward(*head, ptr(ws), nws, _lib.raw_stream(device)),
              "rk_dien_interest_backward")
    else:
        if d_hs is not None and (not d_hs.is_contiguous() or tuple(d_hs.shape) != (batch, T, nh)):
            raise ValueError(f"rankops: d_hs must be a contiguous [{batch}, {T}, {nh}] tensor")
        check(lib.rk_dien_interest_backward_aux(*head, ptr(d_hs), int(bool(accumulate_dkeys)), ptr(ws), nws,
                                                _lib.raw_stream(device)), "rk_dien_interest_backward_aux")
    return grads


DIEN_AUX_MAX_NEG = 8


def dien_aux_loss(hs, keys, seq, neg, neg_seq, seq_len, T, T_neg, H, nh, w_aux, per_sample, mean, batch, device):
    """rk_dien_aux_loss / rk_dien_aux_loss_dense: the auxiliary loss of the extractor states hs
    [batch, T, nh] against the next behaviour and T_neg negatives per step.  Gather form: keys = the
    table [V, H], seq [batch, T], neg_seq [batch, (T-1) T_neg], neg None; dense form: keys [batch, T, H],
    neg [batch, (T-1) T_neg, H], seq / neg_seq None.  Writes per_sample [batch] and mean [1]."""
    lib = _lib.load()
    _lib.ensure_device(device)
    st = _lib.raw_stream(device)
    if seq is not None:
        check(lib.rk_dien_aux_loss(ptr(hs), ptr(keys), keys.shape[0], keys.stride(0), ptr(seq), seq.stride(0),
                                   ptr(neg_seq) if T > 1 else None, neg_seq.stride(0), T, T_neg, ptr(seq_len), batch,
                                   H, nh, ptr(w_aux), ptr(per_sample), ptr(mean), st), "rk_dien_aux_loss")
    else:
        check(lib.rk_dien_aux_loss_dense(ptr(hs), ptr(keys), keys.stride(0), keys.stride(1),
                                         ptr(neg) if T > 1 else None, neg.stride(0), neg.stride(1), T, T_neg,
                                         ptr(seq_len), batch, H, nh, ptr(w_aux), ptr(per_sample), ptr(mean), st),
              "rk_dien_aux_loss_dense")


def dien_aux_loss_backward(hs, keys, seq, neg, neg_seq, seq_len, T, T_neg, H, nh, w_aux, d_loss, batch, device,
                           seq_masked=None, neg_masked=None):
    """rk_dien_aux_loss_backward: sources as dien_aux_loss; d_loss is a one-element device tensor
    (dL/d(mean), read by the kernel).  Returns (d_hs [batch, T, nh], dkeys [batch, T, H], dneg
    [batch, (T-1) T_neg, H], dW_aux [H, nh]), every element written; in the gather form seq_masked
    [batch, T] / neg_masked [batch, (T-1) T_neg] int64, when given, receive the ids with 0 wherever
    dkeys / dneg is zero by masking (the index lists of their embedding scatters)."""
    lib = _lib.load()
    _lib.ensure_device(device)
    f32 = dict(device=device, dtype=torch.float32)
    nneg = (T - 1) * T_neg
    d_hs, dkeys = torch.empty(batch, T, nh, **f32), torch.empty(batch, T, H, **f32)
    dneg, dw = torch.empty(batch, nneg, H, **f32), torch.empty(H, nh, **f32)
    nws = lib.rk_dien_aux_loss_backward_workspace_floats(batch, T, H, nh)
    ws = torch.empty(max(nws, 1), **f32)
    dense = seq is None
    live = T > 1
    check(lib.rk_dien_aux_loss_backward(ptr(hs), ptr(keys), 0 if dense else keys.shape[0],
                                        keys.stride(1) if dense else keys.stride(0), ptr(seq),
                                        0 if dense else seq.stride(0), keys.stride(0) if dense else 0,
                                        ptr(neg) if dense and live else None, neg.stride(0) if dense else 0,
                                        neg.stride(1) if dense else 0, None if dense or not live else ptr(neg_seq),
                                        0 if dense else neg_seq.stride(0), T, T_neg, ptr(seq_len), batch, H, nh,
                                        ptr(w_aux), ptr(d_loss), ptr(d_hs), ptr(dkeys), ptr(dneg) if live else None,
                                        ptr(seq_masked), ptr(neg_masked) if live else None, ptr(dw), ptr(ws), nws,
                                        _lib.raw_stream(device)), "rk_dien_aux_loss_backward")
    return d_hs, dkeys, dneg, dw


def dice_forward(x, scale, shift, alpha, y):
    lib = _lib.load()
    check(lib.rk_dice_forward(ptr(x), x.stride(0), x.shape[0], x.shape[1], ptr(scale), ptr(shift), ptr(alpha),
                              ptr(y), y.stride(0), _lib.stream_of(x)), "rk_dice_forward")


L2_WORKSPACE = 512  # RK_L2_WORKSPACE


def row_l2norm_mean(x: torch.Tensor, col0: int, ncols: int, scale: float, out: torch.Tensor):
    lib = _lib.load()
    ws = torch.empty(L2_WORKSPACE, device=x.device, dtype=torch.float32)
    check(lib.rk_row_l2norm_mean(ptr(x), x.stride(0), x.shape[0], col0, ncols, scale, ptr(ws), ptr(out),
                                 _lib.stream_of(x)), "rk_row_l2norm_mean")
    return out


AFM_LOGIT_SLOT, AFM_PROB_SLOT = 16, 17


def afm_forward_args(fields, dim, batch, dense, dense_w, dense_b, att_w, att_b, att_h, att_hb, p_w, p_b, logit, prob):
    """The argument list of one rk_afm_forward call (the segment array is part of it; the stream
    last); logit / prob (AFM_LOGIT_SLOT / AFM_PROB_SLOT) may be None and patched later."""
    _lib.ensure_device(att_w.device)
    arr = _seg_array(fields)
    nd = dense.shape[1] if dense is not None else 0
    return [arr, len(fields), dim, batch, ptr(dense), dense.stride(0) if dense is not None else 0, nd, ptr(dense_w),
            ptr(dense_b), ptr(att_w), ptr(att_b), att_w.shape[0], ptr(att_h), ptr(att_hb), ptr(p_w), ptr(p_b),
            ptr(logit), ptr(prob), _lib.stream_of(att_w)]


def afm_forward(fields, dim, batch, dense, dense_w, dense_b, att_w, att_b, att_h, att_hb, p_w, p_b, logit, prob):
    check(_lib.load().rk_afm_forward(*afm_forward_args(fields, dim, batch, dense, dense_w, dense_b, att_w, att_b, att_h,
                                                       att_hb, p_w, p_b, logit, prob)), "rk_afm_forward")


def _as_seg_array(segs):
    return segs if isinstance(segs, ctypes.Array) else _seg_array(segs)


FWFM_LOGIT_SLOT, FWFM_PROB_SLOT = 7, 8


def fwfm_forward_args(emb, lin, dim, batch, field_weight, bias, logit, prob):
    """The argument list of one rk_fwfm_forward call (the stream last); emb / lin: lists of Segments or
    ready rk_segment arrays (table_seg_array); logit / prob (FWFM_LOGIT_SLOT / FWFM_PROB_SLOT) may be
    None and patched later."""
    _lib.ensure_device(bias.device)
    return [_as_seg_array(emb), _as_seg_array(lin), len(emb), dim, batch, ptr(field_weight), ptr(bias), ptr(logit),
            ptr(prob), _lib.stream_of(bias)]


def fwfm_forward(emb, lin, dim, batch, field_weight, bias, logit, prob):
    check(_lib.load().rk_fwfm_forward(*fwfm_forward_args(emb, lin, dim, batch, field_weight, bias, logit, prob)),
          "rk_fwfm_forward")


def bst_attention(qkv, batch, T, d_model, heads, seq_len, ctx):
    lib = _lib.load()
    check(lib.rk_bst_attention(ptr(qkv), qkv.stride(0), batch, T, d_model, heads, ptr(seq_len), ptr(ctx),
                               ctx.stride(0), _lib.stream_of(qkv)), "rk_bst_attention")


def bst_attention_masked(qkv, batch, T, d_model, heads, key_mask, ctx):
    """key_mask: None or a [batch, T] uint8 view of the bool key_padding_mask (nonzero = masked)."""
    lib = _lib.load()
    check(lib.rk_bst_attention_masked(ptr(qkv), qkv.stride(0), batch, T, d_model, heads, ptr(key_mask),
                                      key_mask.stride(0) if key_mask is not None else 0, ptr(ctx), ctx.stride(0),
                                      _lib.stream_of(qkv)), "rk_bst_attention_masked")


BST_BLOCK_PARAMS = 17


def bst_forward_blocks(table, seq, seq_len, d_model, heads, blocks, pool_out_ptr, ld_pool, pool_mean,
                       packed=False):
    """rk_bst_forward_blocks: `blocks` = list of (17 device tensors in the header's order,
    (ln1_eps, ln2_eps, slope)); packed: the six projection weights in rk_bst_pack_block_weight's
    layout (rk_bst_forward_blocks_packed)."""
    lib = _lib.load()
    fn, name = ((lib.rk_bst_forward_blocks_packed, "rk_bst_forward_blocks_packed") if packed else
                (lib.rk_bst_forward_blocks, "rk_bst_forward_blocks"))
    B, T = seq.shape
    params = (ctypes.c_void_p * (BST_BLOCK_PARAMS * len(blocks)))()
    scalars = (ctypes.c_float * (3 * len(blocks)))()
    for i, (tensors, sc) in enumerate(blocks):
        assert len(tensors) == BST_BLOCK_PARAMS
        for k, t in enumerate(tensors):
            params[BST_BLOCK_PARAMS * i + k] = ptr(t)
        for k in range(3):
            scalars[3 * i + k] = float(sc[k])
    check(fn(ptr(table), table.shape[0], table.stride(0), ptr(seq), seq.stride(0), T, ptr(seq_len), B, d_model, heads,
             len(blocks), params, scalars, pool_out_ptr, ld_pool, 1 if pool_mean else 0, _lib.stream_of(table)), name)


def pack_bst_weight(weight: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """[128, 128] BST projection weight -> rk_bst_pack_block_weight's MFMA load order (into `out`
    when given: a previous image, rewritten in place)."""
    lib = _lib.load()
    require_gpu(weight, "bst weight")
    if tuple(weight.shape) != (128, 128) or weight.dtype != torch.float32:
        raise ValueError(f"pack_bst_weight: expected a float32 [128, 128] weight, got {tuple(weight.shape)}")
    w = weight.detach().contiguous()
    if out is None:
        out = torch.empty(128, 128, device=w.device, dtype=torch.float32)
    check(lib.rk_bst_pack_block_weight(w.data_ptr(), out.data_ptr(), _lib.stream_of(out)), "rk_bst_pack_block_weight")
    return out


def bst_small_forward_args(segs, width, table, seq, seq_len, heads, blocks, pool_mean, layers, head: Epilogue):
    """The argument list of one rk_bst_small_forward call, the stream last (every array it points
    into is part of the list, so holding it keeps them alive; the tensors stay the caller's)."""
    B, T = seq.shape
    params = (ctypes.c_void_p * (BST_BLOCK_PARAMS * len(blocks)))()
    scalars = (ctypes.c_float * (3 * len(blocks)))()
    for i, (tensors, sc) in enumerate(blocks):
        for k, t in enumerate(tensors):
            params[BST_BLOCK_PARAMS * i + k] = ptr(t)
        for k in range(3):
            scalars[3 * i + k] = float(sc[k])
    arr = _seg_array(segs)
    larr = (_lib.MlpLayer * max(1, len(layers)))(*layers)
    return [arr, len(segs), width, ptr(table), table.shape[0], table.stride(0), ptr(seq), seq.stride(0), T,
            ptr(seq_len), B, heads, len(blocks), params, scalars, 1 if pool_mean else 0, larr, len(layers),
            ctypes.byref(head), _lib.stream_of(table)]


def bst_small_forward(args) -> bool:
    """rk_bst_small_forward over bst_small_forward_args' list: the whole BST eval forward at d_model
    16 in one launch.  False (nothing launched) outside its envelope (RK_ERR_UNSUPPORTED), for the
    three-launch path."""
    rc = _lib.load().rk_bst_small_forward(*args)
    if rc == _lib.RK_ERR_UNSUPPORTED:
        return False
    check(rc, "rk_bst_small_forward")
    return True


def bn_fold(mean, var, weight, bias, eps, scale, shift):
    lib = _lib.load()
    check(lib.rk_bn_fold(ptr(mean), ptr(var), ptr(weight), ptr(bias), float(eps), mean.numel(), ptr(scale),
                         ptr(shift), _lib.stream_of(mean)), "rk_bn_fold")


_EPI_PTR_FIELDS = {f for f, t in Epilogue._fields_ if t is ctypes.c_void_p}


def make_epilogue(**kw) -> Epilogue:
    ep = Epilogue()
    for k, v in kw.items():
        if v is None:
            continue
        if k == "act" and isinstance(v, str):
            v = ACT[v]
        if k in _EPI_PTR_FIELDS and isinstance(v, torch.Tensor):
            v = v.data_ptr()
        setattr(ep, k, v)
    return ep


_MLP_PTR_FIELDS = {f for f, t in _lib.MlpLayer._fields_ if t is ctypes.c_void_p}


def pack_mlp_weight(weight: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """[n, k] nn.Linear weight -> the zero-padded [pad64(n), pad64(k)] layout rk_mlp_forward reads
    (into `out` when given: a previous image of the same weight shape, rewritten in place)."""
    lib = _lib.load()
    n, k = weight.shape
    rows, cols = (n + 63) // 64 * 64, (k + 63) // 64 * 64  # rk_mlp_packed_size
    if out is None or tuple(out.shape) != (rows, cols) or out.device != weight.device:
        out = torch.empty(rows, cols, device=weight.device, dtype=torch.float32)
    w = weight.detach()
    if w.stride(1) != 1:
        w = w.contiguous()
    check(lib.rk_mlp_pack_weight(w.data_ptr(), w.stride(0), n, k, out.data_ptr(), _lib.stream_of(out)),
          "rk_mlp_pack_weight")
    return out


def make_mlp_layer(weight: torch.Tensor, packed: torch.Tensor, **kw) -> "_lib.MlpLayer":
    """One fused-MLP layer: `weight` the [n, k] parameter (n is taken from it), `packed` its
    pack_mlp_weight() image."""
    L = _lib.MlpLayer()
    L.w, L.ldw, L.n = packed.data_ptr(), packed.stride(0), weight.shape[0]
    for k, v in kw.items():
        if v is None:
            continue
        if k == "act" and isinstance(v, str):
            v = ACT[v]
        if k in _MLP_PTR_FIELDS and isinstance(v, torch.Tensor):
            v = v.data_ptr()
        setattr(L, k, v)
    return L


def mlp_forward(x: torch.Tensor, layers, head: Epilogue = None, out: torch.Tensor = None, *, K0: int = None):
    """Whole MLP tail (all hidden layers + optional Linear(N,1)+sigmoid head) in one launch."""
    lib = _lib.load()
    arr = (_lib.MlpLayer * max(1, len(layers)))(*layers)
    K0 = x.shape[1] if K0 is None else K0
    check(lib.rk_mlp_forward(x.data_ptr(), x.stride(0), x.shape[0], K0, arr, len(layers),
                             ctypes.byref(head) if head is not None else None, ptr(out),
                             out.stride(0) if out is not None else 0, _lib.stream_of(x)), "rk_mlp_forward")
    return out


def mlp_forward_gather_args(segs, width, batch, layers, head: Epilogue, device):
    """The rk_mlp_forward_gather argument list (the row gather inside the fused MLP's launch; the
    stream last, None)."""
    _lib.ensure_device(device)
    return [_seg_array(segs), len(segs), width, batch, (_lib.MlpLayer * len(layers))(*layers), len(layers),
            ctypes.byref(head), None]


def linear_tiled(x: torch.Tensor, layer: "_lib.MlpLayer", out: torch.Tensor, K: int = None):
    """One packed MLP layer as a 2D-tiled GEMM (rk_linear_tiled) into `out` [M, n]."""
    lib = _lib.load()
    K = x.shape[1] if K is None else K
    check(lib.rk_linear_tiled(x.data_ptr(), x.stride(0), x.shape[0], K, ctypes.byref(layer), out.data_ptr(),
                              out.stride(0), _lib.stream_of(x)), "rk_linear_tiled")
    return out


_DIN_L2_WS = {}


def _din_l2_workspace(device, batch):
    """rk_din_forward's l2 workspace: ceil(batch/16) partials + a completion counter that starts at
    zero and that every launch leaves at zero, so it is allocated (zeroed) once per device and
    size and reused, also by a hipGraph captured after a warm-up call.  Eager DIN forwards of one
    batch size on one device therefore must not run concurrently on two streams (prepared plans
    carry their own: din_forward_plan)."""
    n = (batch + 15) // 16 + 1
    key = (str(torch.device(device)), n)
    ws = _DIN_L2_WS.get(key)
    if ws is None:
        ws = torch.zeros(n, device=device, dtype=torch.float32)
        _DIN_L2_WS[key] = ws
    return ws


def din_pack_attention(att_weights, H: int) -> torch.Tensor:
    """rk_din_pack_attention: the split attention weights as din_forward_kernel's LDS image."""
    lib = _lib.load()
    w1, b1, w2, b2, w3, _ = att_weights
    _lib.ensure_device(w1.device)
    n = lib.rk_din_attention_image_floats(H)
    if n <= 0:
        raise ValueError(f"rankops.din_pack_attention: H={H} not in (8, 16, 32)")
    img = torch.empty(n, device=w1.device, dtype=torch.float32)
    check(lib.rk_din_pack_attention(ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(w3), H, ptr(img),
                                    _lib.stream_of(img)), "rk_din_pack_attention")
    return img


# rk_din_forward argument slots: the row width, the layer array and its length (pack_epilogue_image),
# and what a cached eager forward patches per call: the six H2 attention weights, l2_out, the image
DIN_WIDTH_SLOT, DIN_LAYERS_SLOT, DIN_NUM_LAYERS_SLOT = 2, 21, 22
DIN_H2_SLOTS, DIN_L2_OUT_SLOT, DIN_ATT_IMAGE_SLOT = slice(14, 20), 27, 28


def _din_forward_args(segs, width, q_col, att_col, key_table, seq, seq_len, H, use_softmax, layers, head: Epilogue,
                      batch, device, l2_col0, l2_scale, want_l2, private_ws=False):
    """The rk_din_forward argument list (without the stream) and the ctypes arrays it points into.
    The H2 weights, l2_out (with want_l2) and the attention image are left empty: the caller patches
    them (DIN_H2_SLOTS, DIN_L2_OUT_SLOT, DIN_ATT_IMAGE_SLOT).  private_ws: an l2 workspace of its own
    (a prepared plan, which may run concurrently with other plans on other streams) instead of the
    shared per-(device, batch) one."""
    _lib.ensure_device(device)
    arr = _seg_array(segs)
    larr = (_lib.MlpLayer * max(1, len(layers)))(*layers)
    ws = None
    if want_l2:
        if private_ws:
            ws = torch.zeros((batch + 15) // 16 + 1, device=device, dtype=torch.float32)
            torch.cuda.current_stream(ws.device).synchronize()  # zeroed before a launch on any stream
        else:
            ws = _din_l2_workspace(device, batch)
    args = [arr, len(segs), width, q_col, att_col, ptr(key_table), key_table.shape[0], key_table.stride(0), ptr(seq),
            seq.stride(0), seq.shape[1], ptr(seq_len), batch, H, None, None, None, None, None, None,
            1 if use_softmax else 0, larr, len(layers), ctypes.byref(head), l2_col0, float(l2_scale),
            ptr(ws), None, None]
    return args, (arr, larr, head, ws)


def din_forward(name, args):
    """Whole DIN eval forward (row gather, attention, fcn tail, head, l2 partials) in one launch:
    `name` is rk_din_forward over _din_forward_args' list + [stream], or rk_din_forward_ex over that
    list + [epilogue image, stream]."""
    check(getattr(_lib.load(), name)(*args), "rk_din_forward")


def pack_epilogue_image(larr, nlayers, K0, device):
    """The per-column epilogue parameters of a layer stack with a compiled streamed plan, packed
    in the streamed tail's LDS layout (rk_mlp_pack_epilogue), or None (no plan;
    RANKOPS_DIN_EPI_DMA=0: the DIN kernel resolves them per column at launch instead)."""
    lib = _lib.load()
    n = lib.rk_mlp_epilogue_image_floats(larr, nlayers, K0)
    if n <= 0 or os.environ.get("RANKOPS_DIN_EPI_DMA", "1") == "0":
        return None
    img = torch.empty(n, device=device, dtype=torch.float32)
    check(lib.rk_mlp_pack_epilogue(larr, nlayers, K0, img.data_ptr(), _lib.raw_stream(device)), "rk_mlp_pack_epilogue")
    return img


class DinPlan:
    """rk_din_forward_plan: the fused DIN forward with its arguments validated once; calling it
    launches the kernel on the current stream (one launch, no per-call host work besides the
    ctypes call).  Binds the pointers it was made with — `keep` holds every tensor it reads or
    writes alive for the plan's lifetime."""

    def __init__(self, args, keep, device):
        self._lib = _lib.load()
        self._device = device
        self._handle = ctypes.c_void_p()
        check(self._lib.rk_din_forward_plan(*args, ctypes.byref(self._handle)), "rk_din_forward_plan")
        self._keep = keep
        self._epi = None
        # phase B's epilogue parameters packed once (rk_mlp_pack_epilogue) and copied into LDS by
        # the kernel, for plans whose launches use them (balanced streamed plans); the image is a
        # snapshot of the current BatchNorm / Dice parameters, as the plan binds the weights
        img = pack_epilogue_image(args[DIN_LAYERS_SLOT], args[DIN_NUM_LAYERS_SLOT], args[DIN_WIDTH_SLOT], device)
        if img is not None and self._lib.rk_din_plan_set_epilogue_image(self._handle, img.data_ptr()) == _lib.RK_OK:
            self._epi = img  # (RK_ERR_UNSUPPORTED: no streamed phase B)

    def launch(self):
        check(self._lib.rk_din_plan_launch(self._handle, _lib.raw_stream(self._device)),
              "rk_din_plan_launch")

    def launch_on(self, stream: int):
        """Launch on an explicit HIP stream (a raw handle, e.g. `torch.cuda.Stream().cuda_stream`),
        without making it the current stream."""
        check(self._lib.rk_din_plan_launch(self._handle, ctypes.c_void_p(stream)), "rk_din_plan_launch")

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            self._lib.rk_din_plan_destroy(h)
            h.value = None


def din_forward_plan(args, keep, device):
    """A DinPlan over _din_forward_args' list (made with private_ws=True, every pointer patched in)."""
    return DinPlan(args, keep, device)


def linear(x: torch.Tensor, weight: torch.Tensor, out: torch.Tensor = None, *, M: int = None, K: int = None,
           x_ptr: int = None, ldx: int = None, x_periodic: torch.Tensor = None, x_period: int = 0,
           y_ptr: int = None, ldy: int = None, epilogue: Epilogue = None):
    """y = epilogue(x . weight^T) on FP32 MFMA.  weight is [N, K] (nn.Linear layout)."""
    lib = _lib.load()
    N = weight.shape[0]
    K = weight.shape[1] if K is None else K
    M = x.shape[0] if M is None else M
    if weight.stride(1) != 1:
        raise ValueError("rankops.linear: weight needs unit column stride")
    xp = x.data_ptr() if x_ptr is None else x_ptr
    lx = x.stride(0) if ldx is None else ldx
    if y_ptr is None and out is not None:
        y_ptr, ldy = out.data_ptr(), out.stride(0) if ldy is None else ldy
    ep = epilogue if epilogue is not None else Epilogue()
    check(lib.rk_linear(xp, lx, ptr(x_periodic), x_period, weight.data_ptr(), weight.stride(0), M, N, K,
                        ctypes.byref(ep), y_ptr, ldy or 0, _lib.stream_of(x)), "rk_linear")
    return out


# ---------------------------------------------------------------- training (§8(f) #2)

_WS_FLOATS = {}
_WS = {}


def _wgrad_ws_floats(lib, M, N, R):
    key = (M, N, R)
    n = _WS_FLOATS.get(key)
    if n is None:
        n = _WS_FLOATS[key] = lib.rk_gemm_wgrad_workspace_floats(M, N, R)
    return n


def _wgrad_workspace(nws: int, device, stream: int) -> torch.Tensor:
    """rk_gemm_wgrad scratch: one buffer per (device, stream) reused by every eager call (calls on
    one stream are ordered, and a launch reads only what it wrote); under stream capture a fresh
    allocation from the graph's pool, so a replay never shares scratch with eager work."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nws, device=device, dtype=torch.float32)
    key = (device, stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nws:
        ws = _WS[key] = torch.empty(max(nws, 1 << 16), device=device, dtype=torch.float32)
    return ws


def gemm(trans_a: bool, trans_b: bool, M: int, N: int, R: int, A: torch.Tensor, lda: int, B: torch.Tensor, ldb: int,
         C: torch.Tensor, ldc: int = None, *, A_mask: torch.Tensor = None, row_sums: torch.Tensor = None,
         accumulate: bool = False, split: int = 0):
    """C[m, n] (+)= sum_r opA(m, r) opB(n, r) (rk_gemm; layouts in include/rankops.h).  Weight
    gradients (both operands transposed: dW = dZ^T X over the batch rows) go to rk_gemm_wgrad when
    the layout allows it."""
    lib = _lib.load()
    ldc_ = C.stride(0) if ldc is None else ldc
    if (trans_a and trans_b and split <= 0 and R >= 512 and (M | N | lda | ldb | ldc_) % 4 == 0
            and all(t is None or t.data_ptr() % 16 == 0 for t in (A, B, A_mask, C, row_sums))):
        nws = _wgrad_ws_floats(lib, M, N, R)
        st = _lib.stream_of(C)
        ws = _wgrad_workspace(nws, C.device, st)
        check(lib.rk_gemm_wgrad(M, N, R, ptr(A), lda, ptr(A_mask), ptr(B), ldb, ptr(C), ldc_, ptr(row_sums),
                                int(accumulate), ptr(ws), nws, st), "rk_gemm_wgrad")
        return C
    check(lib.rk_gemm(int(trans_a), int(trans_b), M, N, R, ptr(A), lda, ptr(A_mask), ptr(B), ldb, ptr(C),
                      C.stride(0) if ldc is None else ldc, ptr(row_sums), int(accumulate), split,
                      _lib.stream_of(C)), "rk_gemm")
    return C


def linear_backward(dy: torch.Tensor, x: torch.Tensor, weight: torch.Tensor, *, relu_out: torch.Tensor = None,
                    need_dx: bool = True, dx: torch.Tensor = None):
    """nn.Linear (+ ReLU when relu_out = the layer's post-ReLU output) backward:
    dz = dy * [relu_out > 0]; dW = dz^T x; db = sum_b dz; dx = dz W.  -> (dx, dW, db)."""
    Bsz, N = dy.shape
    K = weight.shape[1]
    if relu_out is not None and (relu_out.shape != dy.shape or relu_out.stride() != dy.stride()):
        raise ValueError("rankops.linear_backward: relu_out must have dy's shape and strides")
    dW = torch.empty(N, K, device=dy.device, dtype=torch.float32)
    db = torch.empty(N, device=dy.device, dtype=torch.float32)
    gemm(True, True, N, K, Bsz, dy, dy.stride(0), x, x.stride(0), dW, A_mask=relu_out, row_sums=db)
    if need_dx:
        if dx is None:
            dx = torch.empty(Bsz, K, device=dy.device, dtype=torch.float32)
        gemm(False, True, Bsz, K, N, dy, dy.stride(0), weight, weight.stride(0), dx, A_mask=relu_out)
    return dx, dW, db


def logit_head_backward(dlogit, dprob, prob, xa, xb, w, dxa, dxb, dw, db, g_out=None):
    lib = _lib.load()
    check(lib.rk_logit_head_backward(ptr(dlogit), ptr(dprob), ptr(prob), xa.shape[0], ptr(xa), xa.stride(0),
                                     xa.shape[1], ptr(xb), xb.stride(0) if xb is not None else 0,
                                     xb.shape[1] if xb is not None else 0, ptr(w), ptr(dxa),
                                     dxa.stride(0) if dxa is not None else 0, ptr(dxb),
                                     dxb.stride(0) if dxb is not None else 0, ptr(dw), ptr(db), ptr(g_out),
                                     _lib.stream_of(xa)), "rk_logit_head_backward")


def relu_backward(dy, y, out, accumulate=False):
    lib = _lib.load()
    if not (dy.is_contiguous() and y.is_contiguous() and out.is_contiguous()) or dy.shape != y.shape != out.shape:
        raise ValueError("rankops.relu_backward: contiguous tensors of one shape expected")
    check(lib.rk_relu_backward(ptr(dy), ptr(y), ptr(out), dy.numel(), int(accumulate), _lib.stream_of(dy)),
          "rk_relu_backward")
    return out


def dcn_cross_backward(x0, cross_w, cross_b, num_layers, dxl, dx0, accumulate=True):
    lib = _lib.load()
    check(lib.rk_dcn_cross_backward(ptr(x0), x0.stride(0), x0.shape[0], x0.shape[1], ptr(cross_w), ptr(cross_b),
                                    num_layers, ptr(dxl), dxl.stride(0), ptr(dx0), dx0.stride(0), int(accumulate),
                                    _lib.stream_of(x0)), "rk_dcn_cross_backward")


def embedding_backward(grad_segs, batch, dx):
    lib = _lib.load()
    check(lib.rk_embedding_backward(_as_seg_array(grad_segs), len(grad_segs), batch, ptr(dx), dx.stride(0),
                                    _lib.stream_of(dx)), "rk_embedding_backward")


def embedding_backward_seq(grad, seq, dx):
    """rk_embedding_backward_seq: grad[seq[b, t]] += dx[b*T + t] with runs of equal consecutive ids
    pre-summed (no sort); False (nothing launched) when the layout does not allow it."""
    B, T = seq.shape
    d = grad.shape[1]
    if (d % 2 or d > 128 or dx.stride(0) % 2 or grad.stride(0) % 2 or seq.stride(1) != 1
            or dx.data_ptr() % 8 or grad.data_ptr() % 8):
        return False
    lib = _lib.load()
    seg = table_segment(grad, seq, 0, idx_stride=seq.stride(0))
    check(lib.rk_embedding_backward_seq(ctypes.byref(seg), B, T, ptr(dx), dx.stride(0), _lib.stream_of(dx)),
          "rk_embedding_backward_seq")
    return True


def embedding_backward_sorted(grad_seg, n, dx):
    """rk_embedding_backward_sorted: one table segment over n index entries (sorted segment-reduce)."""
    lib = _lib.load()
    nbytes = ctypes.c_int64()
    check(lib.rk_embedding_backward_sorted_workspace_size(n, ctypes.byref(nbytes)),
          "rk_embedding_backward_sorted_workspace_size")
    ws = torch.empty(max(1, nbytes.value), device=dx.device, dtype=torch.uint8)
    check(lib.rk_embedding_backward_sorted(ctypes.byref(grad_seg), n, ptr(dx), dx.stride(0), ptr(ws), nbytes.value,
                                           _lib.stream_of(dx)), "rk_embedding_backward_sorted")


def adam_step(entries, lr, beta1, beta2, eps, weight_decay, step, stream):
    """entries: list of (param, grad, exp_avg, exp_avg_sq[, device step tensor]) float32 tensors."""
    lib = _lib.load()
    arr = (_lib.AdamTensor * len(entries))(*[
        _lib.AdamTensor(e[0].data_ptr(), e[1].data_ptr(), e[2].data_ptr(), e[3].data_ptr(), e[0].numel(),
                        e[4].data_ptr() if len(e) > 4 else None) for e in entries])
    check(lib.rk_adam_step(arr, len(entries), lr, beta1, beta2, eps, weight_decay, step, stream), "rk_adam_step")


def sparse_adam_tensors(entries):
    """rk_sparse_adam_tensor array of entries (param, exp_avg, exp_avg_sq, idx, values, coalesced):
    [rows, dim] float32 tables with unit column stride, idx an int64 vector (any stride), values
    [nnz, dim] float32 rows with unit column stride."""
    arr = (_lib.SparseAdamTensor * max(1, len(entries)))()
    for a, (p, m, v, idx, val, coalesced) in zip(arr, entries):
        rows, dim = p.shape
        nnz = idx.numel()
        if any(t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 for t in (p, m, v)) \
                or m.shape != p.shape or v.shape != p.shape or m.stride() != p.stride() or v.stride() != p.stride():
            raise ValueError("rankops sparse_adam_step: param / exp_avg / exp_avg_sq must be float32 [rows, dim] "
                             "tensors of one layout")
        if idx.dtype != torch.int64 or idx.dim() != 1 or val.dtype != torch.float32 \
                or tuple(val.shape) != (nnz, dim) or (nnz and dim > 1 and val.stride(1) != 1):
            raise ValueError("rankops sparse_adam_step: idx must be an int64 vector and values float32 [nnz, dim]")
        a.param, a.exp_avg, a.exp_avg_sq = p.data_ptr(), m.data_ptr(), v.data_ptr()
        a.rows, a.ld, a.dim = rows, p.stride(0) if rows > 1 else dim, dim
        a.idx, a.idx_stride, a.nnz = idx.data_ptr(), idx.stride(0) if nnz > 1 else 1, nnz
        a.values, a.ld_values = val.data_ptr(), val.stride(0) if nnz > 1 else dim
        a.coalesced = int(bool(coalesced))
    return arr


def sparse_adam_workspace_size(arr, n) -> int:
    nbytes = ctypes.c_int64()
    check(_lib.load().rk_sparse_adam_step_workspace_size(arr, n, ctypes.byref(nbytes)),
          "rk_sparse_adam_step_workspace_size")
    return nbytes.value


_SPARSE_ADAM_ARRAYS = {}


def sparse_adam_step(entries, lr, beta1, beta2, eps, step, stream, device_step=None, workspace=None):
    """rk_sparse_adam_step over entries (see sparse_adam_tensors); `workspace` a uint8 tensor of at
    least the needed size, or None to allocate one.  Returns the workspace used."""
    if not entries:
        return workspace
    # the marshalled array and its workspace size are memoized on every field of the structs, as
    # table_seg_array's are: a repeated step, whose tables, ids and value buffers come back at the
    # same addresses, plans nothing again on the host
    key = tuple((p.data_ptr(), p.shape, p.stride(), m.data_ptr(), v.data_ptr(), i.data_ptr(), i.shape, i.stride(),
                 x.data_ptr(), x.shape, x.stride(), x.dtype, bool(c)) for p, m, v, i, x, c in entries)
    hit = _SPARSE_ADAM_ARRAYS.get(key)
    if hit is None:
        arr = sparse_adam_tensors(entries)
        hit = (arr, sparse_adam_workspace_size(arr, len(entries)))
        if len(_SPARSE_ADAM_ARRAYS) >= 64:
            _SPARSE_ADAM_ARRAYS.clear()
        _SPARSE_ADAM_ARRAYS[key] = hit
    arr, need = hit
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=entries[0][0].device, dtype=torch.uint8)
    check(_lib.load().rk_sparse_adam_step(arr, len(entries), lr, beta1, beta2, eps, int(step), ptr(device_step),
                                          ptr(workspace), workspace.numel(), stream), "rk_sparse_adam_step")
    return workspace


def pack_blocks(blocks, stream):
    """rk_pack_blocks: blocks (src tensor, first column, dst [rows, dim] contiguous[, add tensor]) —
    dst = the dim columns of src's rows from that column on (plus the same columns of add's rows
    when given), every block in one launch."""
    if not blocks:
        return
    arr = (_lib.PackBlock * len(blocks))()
    for a, (src, col, dst, *add) in zip(arr, blocks):
        a.src, a.dst = fptr(src, col), dst.data_ptr()
        a.ld_src, a.rows, a.dim = src.stride(0), dst.shape[0], dst.shape[1]
        if add and add[0] is not None:
            a.add, a.ld_add = fptr(add[0], col), add[0].stride(0)
    check(_lib.load().rk_pack_blocks(arr, len(blocks), stream), "rk_pack_blocks")


def rng_next(counter: torch.Tensor, slot: torch.Tensor):
    lib = _lib.load()
    check(lib.rk_rng_next(ptr(counter), ptr(slot), _lib.stream_of(counter)), "rk_rng_next")


def dropout_mask(seed: int, slot: torch.Tensor, batch: int, n: int, p: float) -> torch.Tensor:
    lib = _lib.load()
    out = torch.empty(batch, n, device=slot.device, dtype=torch.float32)
    check(lib.rk_dropout_mask(seed, ptr(slot), batch, n, p, ptr(out), _lib.stream_of(out)), "rk_dropout_mask")
    return out


def _act_code(act):
    """True/False (ReLU or none) or an ACT name."""
    if isinstance(act, str):
        return ACT[act]
    return _lib.RK_ACT_RELU if act else _lib.RK_ACT_NONE


def _stats_updated(bn):
    """After a train-mode kernel updated `bn`'s running statistics through raw pointers: count the
    batch as torch's BatchNorm does and bump the buffers' versions so eval-mode folds
    (common.FoldedBN) keyed on them recompute."""
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    torch.autograd.graph.increment_version([bn.running_mean, bn.running_var])


def bn_act_train_forward(z, bias, bn, act, p, seed, slot, y, save_mean, save_invstd, workspace, slope=0.0):
    """bn: an nn.BatchNorm1d (train mode) or None; act: True (ReLU), False, or 'leaky' with `slope`."""
    lib = _lib.load()
    track = bn is not None and bn.track_running_stats and bn.running_mean is not None
    check(lib.rk_bn_act_train_forward(
        ptr(z), z.stride(0), z.shape[0], z.shape[1], ptr(bias), int(bn is not None),
        ptr(bn.weight) if bn is not None else None, ptr(bn.bias) if bn is not None else None,
        float(bn.eps) if bn is not None else 0.0, float(bn.momentum) if bn is not None else 0.0,
        ptr(bn.running_mean) if track else None, ptr(bn.running_var) if track else None, ptr(workspace),
        ptr(save_mean), ptr(save_invstd), _act_code(act), float(slope), float(p), seed, ptr(slot), ptr(y),
        y.stride(0), _lib.stream_of(z)), "rk_bn_act_train_forward")
    if track:
        _stats_updated(bn)


def bn_act_backward(dy, z, bias, bn, act, p, seed, slot, save_mean, save_invstd, workspace, dz, dgamma, dbeta,
                    slope=0.0):
    lib = _lib.load()
    check(lib.rk_bn_act_backward(
        ptr(dy), dy.stride(0), ptr(z), z.stride(0), z.shape[0], z.shape[1], ptr(bias), int(bn is not None),
        ptr(bn.weight) if bn is not None else None, ptr(bn.bias) if bn is not None else None, ptr(save_mean),
        ptr(save_invstd), _act_code(act), float(slope), float(p), seed, ptr(slot), ptr(workspace), ptr(dz), dz.stride(0), ptr(dgamma),
        ptr(dbeta), _lib.stream_of(dy)), "rk_bn_act_backward")


def dice_train_forward(z, bias, dice, y, save_mean, save_invstd, workspace):
    """Dice (din.py:26-36) with batch statistics on z + bias; `dice` is the Dice module (its .bn
    running statistics and num_batches_tracked are updated as torch's train-mode BatchNorm does)."""
    lib = _lib.load()
    bn = dice.bn
    track = bn.track_running_stats and bn.running_mean is not None
    check(lib.rk_dice_train_forward(ptr(z), z.stride(0), z.shape[0], z.shape[1], ptr(bias), ptr(dice.alpha),
                                    float(bn.eps), float(bn.momentum), ptr(bn.running_mean) if track else None,
                                    ptr(bn.running_var) if track else None, ptr(workspace), ptr(save_mean),
                                    ptr(save_invstd), ptr(y), y.stride(0), _lib.stream_of(z)), "rk_dice_train_forward")
    if track:
        _stats_updated(bn)


def dice_backward(dy, z, bias, dice, save_mean, save_invstd, workspace, dz, dalpha):
    lib = _lib.load()
    check(lib.rk_dice_backward(ptr(dy), dy.stride(0), ptr(z), z.stride(0), z.shape[0], z.shape[1], ptr(bias),
                               ptr(dice.alpha), ptr(save_mean), ptr(save_invstd), ptr(workspace), ptr(dz),
                               dz.stride(0), ptr(dalpha), _lib.stream_of(dy)), "rk_dice_backward")


def prelu_train_forward(z, bias, prelu, y):
    """nn.PReLU (din.py:277-279) on z + bias; `prelu` is the module (its weight stays on the device)."""
    lib = _lib.load()
    w = prelu.weight
    check(lib.rk_prelu_train_forward(ptr(z), z.stride(0), z.shape[0], z.shape[1], ptr(bias), ptr(w), w.numel(),
                                     ptr(y), y.stride(0), _lib.stream_of(z)), "rk_prelu_train_forward")


def prelu_backward(dy, z, bias, prelu, workspace, dz, dweight):
    lib = _lib.load()
    w = prelu.weight
    check(lib.rk_prelu_backward(ptr(dy), dy.stride(0), ptr(z), z.stride(0), z.shape[0], z.shape[1], ptr(bias), ptr(w),
                                w.numel(), ptr(workspace), ptr(dz), dz.stride(0), ptr(dweight), _lib.stream_of(dy)),
          "rk_prelu_backward")


def din_att_cross(x, q_col, key_table, seq, T, H, keys, cross):
    lib = _lib.load()
    check(lib.rk_din_att_cross(ptr(x), x.stride(0), q_col, ptr(key_table), key_table.shape[0], key_table.stride(0),
                               ptr(seq), seq.stride(0), x.shape[0], T, H, ptr(keys), ptr(cross),
                               _lib.stream_of(x)), "rk_din_att_cross")


def din_att_pool_forward(a2, w3, b3, keys, seq_len, T, H, softmax, weights, x, att_col):
    lib = _lib.load()
    check(lib.rk_din_att_pool_forward(ptr(a2), a2.shape[1], ptr(w3), ptr(b3), ptr(keys), ptr(seq_len), x.shape[0],
                                      T, H, int(bool(softmax)), ptr(weights), ptr(x), x.stride(0), att_col,
                                      _lib.stream_of(x)), "rk_din_att_pool_forward")


def din_att_pool_backward(dx, att_col, weights, keys, a2, w3, seq_len, T, H, softmax, dkeys, da2):
    lib = _lib.load()
    check(lib.rk_din_att_pool_backward(ptr(dx), dx.stride(0), att_col, ptr(weights), ptr(keys), ptr(a2),
                                       a2.shape[1], ptr(w3), ptr(seq_len), dx.shape[0], T, H, int(bool(softmax)),
                                       ptr(dkeys), ptr(da2), _lib.stream_of(dx)), "rk_din_att_pool_backward")


def din_cross_fold(dcross, x, q_col, keys, T, H, dkeys, dx):
    lib = _lib.load()
    check(lib.rk_din_cross_fold(ptr(dcross), ptr(x), x.stride(0), q_col, ptr(keys), x.shape[0], T, H, ptr(dkeys),
                                ptr(dx), dx.stride(0), _lib.stream_of(dx)), "rk_din_cross_fold")


def row_l2norm_backward(x, col0, ncols, scale, grad_out, dx):
    lib = _lib.load()
    check(lib.rk_row_l2norm_backward(ptr(x), x.stride(0), x.shape[0], col0, ncols, float(scale), ptr(grad_out),
                                     ptr(dx), dx.stride(0), _lib.stream_of(dx)), "rk_row_l2norm_backward")


def fwfm_backward(emb_segs, dim, batch, field_weight, prob, dprob, d_emb, dz, d_field_weight, d_bias):
    lib = _lib.load()
    check(lib.rk_fwfm_backward(_as_seg_array(emb_segs), len(emb_segs), dim, batch, ptr(field_weight), ptr(prob),
                               ptr(dprob), ptr(d_emb), d_emb.stride(0), ptr(dz), ptr(d_field_weight), ptr(d_bias),
                               _lib.stream_of(prob)), "rk_fwfm_backward")


def afm_pairs(fields, dim, batch, emb, pairs):
    lib = _lib.load()
    check(lib.rk_afm_pairs(_seg_array(fields), len(fields), dim, batch, ptr(emb), ptr(pairs), _lib.stream_of(emb)),
          "rk_afm_pairs")


def afm_pool_forward(a1, w2, b2, pairs, num_pairs, dim, dense, wd, bd, wp, bp, weights, ws, logit, pred):
    lib = _lib.load()
    check(lib.rk_afm_pool_forward(ptr(a1), a1.shape[1], ptr(w2), ptr(b2), ptr(pairs), num_pairs, dim, ptr(dense),
                                  dense.stride(0), dense.shape[1], ptr(wd), ptr(bd), ptr(wp), ptr(bp), dense.shape[0],
                                  ptr(weights), ptr(ws), ptr(logit), ptr(pred), _lib.stream_of(pred)),
          "rk_afm_pool_forward")


def afm_pool_backward(dpred, dtotal, pred, weights, ws, pairs, a1, w2, wp, dense, num_pairs, dim, d_pairs, da1, acc):
    lib = _lib.load()
    check(lib.rk_afm_pool_backward(ptr(dpred), ptr(dtotal), ptr(pred), ptr(weights), ptr(ws), ptr(pairs), ptr(a1),
                                   a1.shape[1], ptr(w2), ptr(wp), ptr(dense), dense.stride(0), dense.shape[1],
                                   dense.shape[0], num_pairs, dim, ptr(d_pairs), ptr(da1), ptr(acc),
                                   _lib.stream_of(pred)), "rk_afm_pool_backward")


def afm_pair_fold(d_pairs, emb, num_fields, dim, d_emb):
    lib = _lib.load()
    check(lib.rk_afm_pair_fold(ptr(d_pairs), ptr(emb), num_fields, dim, emb.shape[0], ptr(d_emb),
                               _lib.stream_of(emb)), "rk_afm_pair_fold")


def bst_add_pos(x, pos, T, xp):
    lib = _lib.load()
    check(lib.rk_bst_add_pos(ptr(x), ptr(pos), T, x.shape[0], x.shape[1], ptr(xp), _lib.stream_of(x)),
          "rk_bst_add_pos")


def bst_gather_pos(table, idx, T, pos, x, xp):
    """x = table[idx], xp = x + pos[m % T] in one pass (rk_bst_gather_pos); False when the layout
    does not allow it (nothing launched)."""
    d = table.shape[1]
    if (d % 4 or table.stride(0) % 4 or idx.stride(0) != 1 or pos.stride(0) != d
            or any(t.data_ptr() % 16 for t in (table, pos, x, xp))):
        return False
    lib = _lib.load()
    check(lib.rk_bst_gather_pos(ptr(table), table.shape[0], table.stride(0), ptr(idx), idx.shape[0], T, d, ptr(pos),
                                ptr(x), ptr(xp), _lib.stream_of(x)), "rk_bst_gather_pos")
    return True


def bst_attn_train_forward(qkv, B, T, d, heads, seq_len, probs, ctx):
    lib = _lib.load()
    check(lib.rk_bst_attn_train_forward(ptr(qkv), B, T, d, heads, ptr(seq_len), ptr(probs), ptr(ctx),
                                        _lib.stream_of(qkv)), "rk_bst_attn_train_forward")


def bst_attn_train_backward(qkv, probs, dctx, B, T, d, heads, dqkv):
    lib = _lib.load()
    check(lib.rk_bst_attn_train_backward(ptr(qkv), ptr(probs), ptr(dctx), B, T, d, heads, ptr(dqkv),
                                         _lib.stream_of(qkv)), "rk_bst_attn_train_backward")


def linear_res_dropout_ln(x, weight, bias, base, p, seed, slot, ln, r, y, mean, rstd) -> bool:
    """rk_linear_res_dropout_ln: y = LayerNorm(base + dropout(x W^T + bias)) in one launch; False
    (nothing launched) when the shape is not the fused kernel's (d_model != 128, K, alignment, M)."""
    d = weight.shape[0]
    if (d != 128 or weight.shape[1] != x.shape[1] or weight.stride(1) != 1 or x.stride(1) != 1
            or not all(t.is_contiguous() for t in (base, r, y)) or ln.weight is None or ln.bias is None):
        return False
    lib = _lib.load()
    rc = lib.rk_linear_res_dropout_ln(ptr(x), x.stride(0), x.shape[0], x.shape[1], ptr(weight), weight.stride(0),
                                      ptr(bias), ptr(base), float(p), seed, ptr(slot), ptr(ln.weight), ptr(ln.bias),
                                      float(ln.eps), ptr(r), ptr(y), ptr(mean), ptr(rstd), _lib.stream_of(x))
    if rc == _lib.RK_ERR_UNSUPPORTED:
        return False
    check(rc, "rk_linear_res_dropout_ln")
    return True


def bst_res_dropout_ln_forward(base, o, p, seed, slot, ln, r, y, mean, rstd):
    lib = _lib.load()
    check(lib.rk_bst_res_dropout_ln_forward(ptr(base), ptr(o), base.shape[0], base.shape[1], float(p), seed,
                                            ptr(slot), ptr(ln.weight), ptr(ln.bias), float(ln.eps), ptr(r), ptr(y),
                                            ptr(mean), ptr(rstd), _lib.stream_of(base)),
          "rk_bst_res_dropout_ln_forward")


def bst_ln_backward(dy, r, mean, rstd, ln, p, seed, slot, dr, d_o, dgamma, dbeta):
    lib = _lib.load()
    nws = lib.rk_bst_ln_backward_workspace_floats(r.shape[1])
    ws = torch.empty(nws, device=r.device, dtype=torch.float32)
    check(lib.rk_bst_ln_backward(ptr(dy), ptr(r), ptr(mean), ptr(rstd), ptr(ln.weight), r.shape[0], r.shape[1],
                                 float(p), seed, ptr(slot), ptr(dr), ptr(d_o), ptr(dgamma), ptr(dbeta), ptr(ws),
                                 nws, _lib.stream_of(dy)), "rk_bst_ln_backward")


def bst_pool_ln_backward(drow, col, T, seq_len, mean_pool, r, mean, rstd, ln, p, seed, slot, dr, d_o, dgamma,
                         dbeta):
    """bst_ln_backward whose incoming gradient is the pooling backward's broadcast of drow
    (rk_bst_pool_ln_backward); returns False (nothing launched) when the layout does not allow it."""
    lib = _lib.load()
    d = r.shape[1]
    if d % 4 or any(t is not None and t.data_ptr() % 16 for t in (r, ln.weight, dr, d_o)):
        return False
    nws = lib.rk_bst_ln_backward_workspace_floats(d)
    ws = torch.empty(nws, device=r.device, dtype=torch.float32)
    check(lib.rk_bst_pool_ln_backward(ptr(drow), drow.stride(0), col, T, ptr(seq_len), int(mean_pool), ptr(r),
                                      ptr(mean), ptr(rstd), ptr(ln.weight), r.shape[0], d, float(p), seed, ptr(slot),
                                      ptr(dr), ptr(d_o), ptr(dgamma), ptr(dbeta), ptr(ws), nws, _lib.stream_of(r)),
          "rk_bst_pool_ln_backward")
    return True


def bst_pos_backward(dxp, B, T, dpos):
    lib = _lib.load()
    check(lib.rk_bst_pos_backward(ptr(dxp), B, T, dxp.shape[1], ptr(dpos), _lib.stream_of(dxp)),
          "rk_bst_pos_backward")


def bst_leaky_dropout(inp, f, slope, p, seed, slot, backward, out):
    lib = _lib.load()
    check(lib.rk_bst_leaky_dropout(ptr(inp), ptr(f), f.numel(), float(slope), float(p), seed, ptr(slot),
                                   int(backward), ptr(out), _lib.stream_of(f)), "rk_bst_leaky_dropout")


def bst_pool(x, B, T, seq_len, mean, row, col):
    lib = _lib.load()
    check(lib.rk_bst_pool(ptr(x), B, T, x.shape[1], ptr(seq_len), int(mean), ptr(row), row.stride(0), col,
                          _lib.stream_of(x)), "rk_bst_pool")


def bst_pool_backward(drow, col, B, T, d, seq_len, mean, dx):
    lib = _lib.load()
    check(lib.rk_bst_pool_backward(ptr(drow), drow.stride(0), col, B, T, d, ptr(seq_len), int(mean), ptr(dx),
                                   _lib.stream_of(dx)), "rk_bst_pool_backward")


def fm_backward(deep_in, d_deep, dfm2, num_fields, dim, out):
    lib = _lib.load()
    check(lib.rk_fm_backward(ptr(deep_in), deep_in.stride(0), ptr(d_deep), d_deep.stride(0) if d_deep is not None else 0,
                             ptr(dfm2), deep_in.shape[0], num_fields, dim, ptr(out), out.stride(0),
                             _lib.stream_of(deep_in)), "rk_fm_backward")


def shard_fm_assemble(recv, num_fields, num_owners, dim, deep_in, fm1, fm2):
    """rk_shard_fm_assemble: the received split-wire blocks of all owners -> deep_in [B, F * dim], fm1, fm2."""
    lib = _lib.load()
    check(lib.rk_shard_fm_assemble(ptr(recv), num_fields, num_owners, dim, deep_in.shape[0], ptr(deep_in),
                                   deep_in.stride(0), ptr(fm1), ptr(fm2), _lib.stream_of(deep_in)),
          "rk_shard_fm_assemble")


def shard_fm_backward_pack(deep_in, d_deep, dfm2, dfm1, scale, num_fields, num_owners, dim, out):
    """rk_shard_fm_backward_pack: scale * the FM backward, written into the gradient send blocks `out`."""
    lib = _lib.load()
    check(lib.rk_shard_fm_backward_pack(ptr(deep_in), deep_in.stride(0), ptr(d_deep),
                                        d_deep.stride(0) if d_deep is not None else 0, ptr(dfm2), ptr(dfm1),
                                        float(scale), deep_in.shape[0], num_fields, num_owners, dim, ptr(out),
                                        _lib.stream_of(deep_in)), "rk_shard_fm_backward_pack")


def shard_unpack_grads(recv, idx, num_fields, dim, num_sources, source_batch, ids, values2, values1):
    """rk_shard_unpack_grads: the received gradient blocks + kept indices -> ids [F, N], values2 [F, N, dim],
    values1 [N] (N = num_sources * source_batch)."""
    lib = _lib.load()
    check(lib.rk_shard_unpack_grads(ptr(recv), ptr(idx), num_fields, dim, num_sources, source_batch, ptr(ids),
                                    ptr(values2), ptr(values1), _lib.stream_of(recv)), "rk_shard_unpack_grads")


def fm_combine_backward(dprob, dtotal, dfm1_in, dfm2_in, ddeep_in, prob, fm1, fm2, deep, final_w, dfm1, dfm2, ddeep,
                        dfinal_w, dfinal_b):
    lib = _lib.load()
    check(lib.rk_fm_combine_backward(ptr(dprob), ptr(dtotal), ptr(dfm1_in), ptr(dfm2_in), ptr(ddeep_in), ptr(prob),
                                     ptr(fm1), ptr(fm2), ptr(deep), ptr(final_w), prob.shape[0], ptr(dfm1), ptr(dfm2),
                                     ptr(ddeep), ptr(dfinal_w), ptr(dfinal_b), _lib.stream_of(prob)),
          "rk_fm_combine_backward")


# ---------------------------------------------------------------- MMoE (rk_mmoe_forward)

# argument slots of rk_mmoe_forward patched per call (mmoe_forward_args)
MMOE_LOGITS_SLOT, MMOE_PROBS_SLOT, MMOE_MIXED_SLOT, MMOE_GATES_SLOT = 14, 15, 16, 17


def _mmoe_layer_array(stacks):
    """[[(image, bias or None, n, act)…]…] -> one rk_mmoe_layer array, stack-major."""
    flat = [l for stack in stacks for l in stack]
    arr = (_lib.MmoeLayer * max(1, len(flat)))()
    for d, (image, bias, n, act) in zip(arr, flat):
        d.w, d.bias, d.n, d.act = image.data_ptr(), ptr(bias), int(n), ACT[act] if isinstance(act, str) else int(act)
    return arr


def mmoe_forward_args(segs, width, batch, experts, gate_image, gate_bias, num_tasks, towers, heads, device, *,
                      logits=None, probs=None, mixed=None, gate_probs=None):
    """The rk_mmoe_forward argument list (the stream last, None) and the ctypes arrays it points into.
    experts: E stacks of equal depth, towers: K stacks of equal depth (or None), each a list of
    (pack_mlp_weight image, bias or None, n, act); gate_image: the image of the K gate weights stacked
    to [K E, width], gate_bias [K E] or None; heads: K (w [last width], b [1]) or None.  logits [14],
    probs [15], mixed [16], gate_probs [17] and the stream [-1] are the per-call slots of a cached
    forward."""
    _lib.ensure_device(device)
    arr = _as_seg_array(segs)
    depth = len(experts[0]) if experts else 0
    if any(len(s) != depth for s in experts):
        raise ValueError("rankops.mmoe: every expert must have the same number of layers")
    ex = _mmoe_layer_array(experts)
    tdepth, tw, hw, hb = 0, None, None, None
    if heads is not None:
        towers = towers if towers is not None else [[] for _ in range(num_tasks)]
        if len(towers) != num_tasks or len(heads) != num_tasks:
            raise ValueError(f"rankops.mmoe: {num_tasks} gates need {num_tasks} towers and heads")
        tdepth = len(towers[0])
        if any(len(s) != tdepth for s in towers):
            raise ValueError("rankops.mmoe: every tower must have the same number of layers")
        tw = _mmoe_layer_array(towers) if tdepth else None
        hw = (ctypes.c_void_p * num_tasks)(*[w.data_ptr() for w, _ in heads])
        hb = (ctypes.c_void_p * num_tasks)(*[b.data_ptr() for _, b in heads])
    args = [arr, len(arr), width, batch, ex, len(experts), depth, gate_image.data_ptr(), ptr(gate_bias), num_tasks,
            tw, tdepth, hw, hb, ptr(logits), ptr(probs), ptr(mixed), ptr(gate_probs), None]
    return args, (arr, ex, tw, hw, hb)


def _mmoe_stack(layers, k_in, what, pack=True):
    """[(W, b)…] -> ([(image, bias, n, 'relu')…], output width), every Linear followed by ReLU.  pack=False
    (an empty batch: nothing is launched) checks the shapes and leaves the images None."""
    out = []
    for l, (w, b) in enumerate(layers):
        as_f32(w, f"{what} layer {l} weight")
        if w.dim() != 2 or w.shape[1] != k_in:
            raise ValueError(f"rankops.mmoe: {what} layer {l} weight must be [n, {k_in}], got {tuple(w.shape)}")
        if b is not None and (as_f32(b, f"{what} layer {l} bias").dim() != 1 or b.shape[0] != w.shape[0]
                              or not b.is_contiguous()):
            raise ValueError(f"rankops.mmoe: {what} layer {l} bias must be a contiguous [{w.shape[0]}] tensor")
        out.append((pack_mlp_weight(w) if pack else None, b.detach() if b is not None else None, w.shape[0], "relu"))
        k_in = w.shape[0]
    return out, k_in


# ---------------------------------------------------------------- MMoE training ("Training")

def p4(v: int) -> int:
    return (v + 3) // 4 * 4


def _ptrs(values):
    return (ctypes.c_void_p * len(values))(*values)


def pack_mlp_weights(pairs, stream):
    """rk_mlp_pack_weights: [(weight [n, k] with unit column stride, image [pad64(n), pad64(k)])…], one launch."""
    if not pairs:
        return
    arr = (_lib.PackItem * len(pairs))()
    for it, (w, out) in zip(arr, pairs):
        it.w, it.out, it.ldw, it.n, it.k = w.data_ptr(), out.data_ptr(), w.stride(0), w.shape[0], w.shape[1]
    check(_lib.load().rk_mlp_pack_weights(arr, len(pairs), stream), "rk_mlp_pack_weights")


def mlp_image(n, k, device):
    return torch.empty((n + 63) // 64 * 64, (k + 63) // 64 * 64, device=device, dtype=torch.float32)


def gemm_grouped(trans_a, trans_b, M, N, R, A, lda, B, ldb, C, ldc, stream, *, C_mask=None, ldmask=0, mask_scale=1.0,
                 accumulate=False):
    """rk_gemm_grouped; A, B, C, C_mask are lists of device addresses (fptr), one per group."""
    check(_lib.load().rk_gemm_grouped(len(C), int(trans_a), int(trans_b), M, N, R, _ptrs(A), lda, _ptrs(B), ldb,
                                      _ptrs(C), ldc, _ptrs(C_mask) if C_mask is not None else None, ldmask,
                                      mask_scale, int(accumulate), stream), "rk_gemm_grouped")


def gemm_wgrad_grouped(N, K, R, A, lda, B, ldb, C, ldc, row_sums, device, stream, accumulate=False):
    """rk_gemm_wgrad_grouped over lists of device addresses, with the shared wgrad workspace."""
    lib = _lib.load()
    G = len(C)
    nws = lib.rk_gemm_wgrad_grouped_workspace_floats(G, N, K, R)
    ws = _wgrad_workspace(nws, device, stream)
    check(lib.rk_gemm_wgrad_grouped(G, N, K, R, _ptrs(A), lda, _ptrs(B), ldb, _ptrs(C), ldc,
                                    _ptrs(row_sums) if row_sums is not None else None, int(accumulate), ptr(ws),
                                    ws.numel(), stream), "rk_gemm_wgrad_grouped")


def mmoe_mix_backward(B, E, K, H, dmixed, ld_dm, pitch_dm, f, ld_f, pitch_f, gate_probs, mask_scale, dgl, ld_dgl, dz,
                      ld_dz, pitch_dz, stream):
    """rk_mmoe_mix_backward; dmixed, f, dgl, dz are device addresses or tensors."""
    a = [t.data_ptr() if isinstance(t, torch.Tensor) else t for t in (dmixed, f, gate_probs, dgl, dz)]
    check(_lib.load().rk_mmoe_mix_backward(B, E, K, H, a[0], ld_dm, pitch_dm, a[1], ld_f, pitch_f, a[2], mask_scale,
                                           a[3], ld_dgl, a[4], ld_dz, pitch_dz, stream), "rk_mmoe_mix_backward")


def mmoe_head_backward(B, K, n, pitch, dlogits, dprobs, probs, head_w, t, mask_scale, g_out, dt, accumulate, stream):
    check(_lib.load().rk_mmoe_head_backward(B, K, n, pitch, ptr(dlogits), ptr(dprobs), ptr(probs),
                                            _ptrs([w.data_ptr() for w in head_w]), ptr(t), mask_scale, ptr(g_out),
                                            g_out.stride(0), ptr(dt), int(accumulate), stream),
          "rk_mmoe_head_backward")


class MmoeShape:
    """Widths of one MMoE: the row, E experts of units eu, K tasks with towers of units tu."""

    def __init__(self, width, E, K, eu, tu, heads: bool):
        self.width, self.E, self.K, self.eu, self.tu, self.heads = width, E, K, tuple(eu), tuple(tu), heads
        self.H = self.eu[-1]
        # a width off the 4 grid: its buffers are padded to the grid (the forward and the backward kernels
        # write zeros there) and its gradients are cut out of padded results
        self.padded = any(v % 4 for v in (width, E * K) + self.eu + self.tu)
        self.zw = E * p4(self.eu[0]) + p4(K * E)   # columns of dZ0 = [dz_{0,0} | … | dz_{E-1,0} | dgate_logits]
        self.zw_padded = self.zw != E * self.eu[0] + K * E   # dZ0 has pad columns of its own (zero-filled)


def mmoe_stacked_weight(sh: MmoeShape, experts, gates):
    """[W_{0,0}; …; W_{E-1,0}; W_gate_0; …] as one [zw, p4(width)] matrix (rows and columns on the 4 grid,
    zeros between): layer 0 of every expert and the K gates read the same x, so their data gradient is
    one GEMM against it, their weight gradients one product, and its tail is the stacked gate weight."""
    first = [layers[0][0].detach() for layers in experts] + [w.detach() for w, _ in gates]
    pad = torch.nn.functional.pad
    cols = p4(sh.width) - sh.width
    if not sh.zw_padded:  # rows already on the grid: one cat, one pad of the columns if the width is off it
        out = torch.cat(first, 0)
        return pad(out, (0, cols)) if cols else out
    # (a fixed number of launches whatever E and K: stack, pad, cat, pad, cat)
    n0, KE = sh.eu[0], sh.K * sh.E
    top = pad(torch.stack(first[:sh.E], 0), (0, cols, 0, p4(n0) - n0)).view(sh.E * p4(n0), p4(sh.width))
    tail = pad(torch.cat(first[sh.E:], 0), (0, cols, 0, p4(KE) - KE))
    return torch.cat([top, tail], 0)


def mmoe_forward_train(segs, sh: MmoeShape, B, stacks, gate_image, gate_bias, tstacks, heads, device, p, seed, slot):
    """rk_mmoe_forward_train: one launch; returns the saved buffers (include/rankops.h) as a dict."""
    new = torch.empty  # (the kernel writes the pad columns)
    f32 = dict(device=device, dtype=torch.float32)
    E, K = sh.E, sh.K
    s = dict(x=new(B, p4(sh.width), **f32), eacts=[new(B, E * p4(n), **f32) for n in sh.eu],
             tacts=[new(B, K * p4(n), **f32) for n in sh.tu], mixed=new(B, K * p4(sh.H), **f32),
             gate_probs=torch.empty(B, K, E, **f32), logits=None, probs=None)
    if heads is not None:
        s["logits"], s["probs"] = torch.empty(B, K, **f32), torch.empty(B, K, **f32)
    if B == 0:
        return s
    args, keep = mmoe_forward_args(segs, sh.width, B, stacks, gate_image, gate_bias, K, tstacks, heads, device)
    ea = _ptrs([t.data_ptr() for t in s["eacts"]])
    ta = _ptrs([t.data_ptr() for t in s["tacts"]]) if sh.tu else None
    call = args[:14] + [float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(slot), s["x"].data_ptr(), ea, ta, ptr(s["logits"]),
                        ptr(s["probs"]), s["mixed"].data_ptr(), s["gate_probs"].data_ptr(), _lib.raw_stream(device)]
    check(_lib.load().rk_mmoe_forward_train(*call), "rk_mmoe_forward_train")
    return s


def _wgrad(B, N, Kd, A, lda, Bm, ldb, device, st):
    """One rk_gemm_wgrad over the B rows: (dW [N, Kd] = A^T Bm, db [N] = A's column sums); A and Bm may be
    column blocks of wider buffers (views: their addresses, lda / ldb the row strides)."""
    lib = _lib.load()
    f32 = dict(device=device, dtype=torch.float32)
    dW, db = torch.empty(N, Kd, **f32), torch.empty(N, **f32)
    nws = _wgrad_ws_floats(lib, N, Kd, B)
    ws = _wgrad_workspace(nws, device, st)
    check(lib.rk_gemm_wgrad(N, Kd, B, A.data_ptr(), lda, None, Bm.data_ptr(), ldb, dW.data_ptr(), Kd, db.data_ptr(), 0,
                            ws.data_ptr(), ws.numel(), st), "rk_gemm_wgrad")
    return dW, db


def mtl_tower_backward(K, H, tu, B, tacts, mixed, probs, towers, scale, d_mixed, d_logits, d_probs, device, st, *,
                       first=0):
    """The heads and towers of a multi-task model (MMoE, PLE), backward: rk_mmoe_head_backward, one
    rk_gemm_wgrad for the heads and per tower layer the grouped pair over the K tasks.  tacts, mixed
    [B, K p4(H)], probs: the train forward's buffers; towers: K (hidden [(W, b)…], (w, b)) or None;
    d_mixed [B, K, H], d_logits, d_probs [B, K]: the incoming gradients, each may be None.  Returns (the
    gradient of the mixtures [B, K p4(H)] — a private buffer —, tower grads [([(dW, db)…], (dw, db))…] or
    None).  first=1 (ESMM: the towers' first layers read one shared row, not per-task mixtures; Dt >= 1,
    mixed = d_mixed = None) stops above layer 0: the first result is then dz_0 [B, K p4(tu[0])], the gradient
    at layer 0's pre-activations with zeros in its pad columns, and every hidden_grads[k][0] is None for
    the caller to fill."""
    tu = tuple(tu)
    Dt = len(tu)
    pt, pm = [p4(n) for n in tu], p4(H)
    f32 = dict(device=device, dtype=torch.float32)
    new = torch.empty

    def wgrad(N, Kd, A, lda, Bm, ldb):
        return _wgrad(B, N, Kd, A, lda, Bm, ldb, device, st)

    def incoming():  # d_mixed [B, K, H] in the saved layout [B, K pm], a private copy (it is added to)
        if pm == H:
            return d_mixed.reshape(B, K * H).clone()
        buf = torch.zeros(B, K, pm, **f32)
        buf[:, :, :H] = d_mixed
        return buf.view(B, K * pm)

    tower_grads = None
    dmix = None
    if towers is not None and (d_logits is not None or d_probs is not None):
        last, plast = (tu[-1], pt[-1]) if Dt else (H, pm)
        feed = tacts[-1] if Dt else mixed            # the heads' input, [B, K plast]
        pk = p4(K)
        g = torch.empty(B, pk, **f32)
        own = Dt == 0 and d_mixed is not None
        dz = incoming() if own else new(B, K * plast, **f32)
        mmoe_head_backward(B, K, last, plast, d_logits, d_probs, probs, [w for _, (w, _) in towers],
                           tacts[-1] if Dt else None, scale, g, dz, own, st)
        hd, hb = wgrad(pk, K * plast, g, pk, feed, K * plast)  # the heads' dw are its diagonal blocks
        head_grads = [(hd[k, k * plast:k * plast + last].view(1, last), hb[k:k + 1]) for k in range(K)]
        hidden_grads = [[None] * Dt for _ in range(K)]
        for l in range(Dt - 1, first - 1, -1):
            n, n_in, p_in = tu[l], (tu[l - 1] if l else H), (pt[l - 1] if l else pm)
            inp = tacts[l - 1] if l else mixed
            dW, db = torch.empty(K, pt[l], p4(n_in), **f32), torch.empty(K, pt[l], **f32)
            gemm_wgrad_grouped(pt[l], p4(n_in), B, [fptr(dz, k * pt[l]) for k in range(K)], K * pt[l],
                               [fptr(inp, k * p_in) for k in range(K)], K * p_in, [dW[k].data_ptr() for k in range(K)],
                               p4(n_in), [db[k].data_ptr() for k in range(K)], device, st)
            dW, db = dW[:, :n, :n_in].contiguous(), db[:, :n].contiguous()  # (no launch unless padded)
            for k in range(K):
                hidden_grads[k][l] = (dW[k], db[k])
            add = l == 0 and d_mixed is not None
            # (dz_0 of first=1 is read whole by the stacked layer-0 products: its pad columns must be zero)
            fill = torch.zeros if first and l == first and p_in != n_in else new
            d_in = incoming() if add else fill(B, K * p_in, **f32)
            ws_ = [towers[k][0][l][0] for k in range(K)]
            gemm_grouped(False, True, B, n_in, n, [fptr(dz, k * pt[l]) for k in range(K)], K * pt[l],
                         [w.data_ptr() for w in ws_], ws_[0].stride(0), [fptr(d_in, k * p_in) for k in range(K)],
                         K * p_in, st, C_mask=[fptr(inp, k * p_in) for k in range(K)] if l else None, ldmask=K * p_in,
                         mask_scale=scale, accumulate=add)
            dz = d_in
        dmix = dz
        tower_grads = [(hidden_grads[k], head_grads[k]) for k in range(K)]
    elif d_mixed is not None:
        dmix = incoming()
    if towers is not None and tower_grads is None:  # the heads saw no gradient
        tower_grads = [([(torch.zeros_like(W), torch.zeros(W.shape[0], **f32)) for W, _ in hidden],
                        (torch.zeros_like(w), torch.zeros(1, **f32))) for hidden, (w, _) in towers]
    if dmix is None:
        dmix = torch.zeros(B, K * pm, **f32)
    return dmix, tower_grads


def mmoe_backward(sh: MmoeShape, B, s, wst, experts, gates, towers, p, d_mixed, d_logits, d_probs, need_dx, device):
    """The MMoE backward from the buffers of mmoe_forward_train (s), the stacked layer-0 / gate weight
    (wst) and the plain weights (experts: E lists of (W, b); gates: K (W, b); towers: K (hidden, (w, b)) or
    None).  d_mixed [B, K, H], d_logits, d_probs [B, K]: the incoming gradients, each may be None.
    Returns (dx [B, width] or None, expert grads [[(dW, db)…]…], gate grads [(dW, db)…], tower grads
    [([(dW, db)…], (dw, db))…] or None); a db is returned for every layer (callers drop those of bias-free
    layers).  The launches do not depend on E or K: per layer one rk_gemm_wgrad_grouped and one
    rk_gemm_grouped over the experts (tasks); layer 0 of all experts and the gates as one rk_gemm_wgrad and
    one rk_gemm; no float atomics, fixed-order sums."""
    E, K, H, width = sh.E, sh.K, sh.H, sh.width
    De, Dt = len(sh.eu), len(sh.tu)
    pe, pm, w4 = [p4(n) for n in sh.eu], p4(H), p4(width)
    f32 = dict(device=device, dtype=torch.float32)
    # Pad columns: the head and mix kernels write zeros into theirs; rk_gemm_grouped leaves those of its
    # outputs unwritten, which only reach rows of padded weight gradients that are cut away (the next
    # grouped GEMM reduces over the exact width).  dZ0's own pad columns are read by the stacked data
    # gradient, so dZ0 is zero-filled when it has any.
    new = torch.empty
    st = _lib.raw_stream(device)
    scale = 1.0 / (1.0 - p)

    def wgrad(N, Kd, A, lda, Bm, ldb):
        return _wgrad(B, N, Kd, A, lda, Bm, ldb, device, st)

    # heads and towers (shared with ple_backward)
    dmix, tower_grads = mtl_tower_backward(K, H, sh.tu, B, s["tacts"], s["mixed"], s["probs"], towers, scale, d_mixed,
                                           d_logits, d_probs, device, st)

    # the mix and the gates' softmax; with one expert layer its dz goes straight into dZ0
    dZ0 = (torch.zeros if sh.zw_padded else torch.empty)(B, sh.zw, **f32)
    if De == 1:
        dz, ld_dz = dZ0, sh.zw
    else:
        dz, ld_dz = new(B, E * pe[-1], **f32), E * pe[-1]
    mmoe_mix_backward(B, E, K, H, dmix, K * pm, pm, s["eacts"][-1], E * pe[-1], pe[-1], s["gate_probs"], scale,
                      fptr(dZ0, E * pe[0]), sh.zw, dz, ld_dz, pe[-1], st)
    expert_grads = [[None] * De for _ in range(E)]
    for l in range(De - 1, 0, -1):
        n, n_in = sh.eu[l], sh.eu[l - 1]
        inp = s["eacts"][l - 1]
        dW, db = torch.empty(E, pe[l], pe[l - 1], **f32), torch.empty(E, pe[l], **f32)
        gemm_wgrad_grouped(pe[l], pe[l - 1], B, [fptr(dz, e * pe[l]) for e in range(E)], ld_dz,
                           [fptr(inp, e * pe[l - 1]) for e in range(E)], E * pe[l - 1],
                           [dW[e].data_ptr() for e in range(E)], pe[l - 1], [db[e].data_ptr() for e in range(E)],
                           device, st)
        dW, db = dW[:, :n, :n_in].contiguous(), db[:, :n].contiguous()
        for e in range(E):
            expert_grads[e][l] = (dW[e], db[e])
        if l == 1:
            d_in, ld_in = dZ0, sh.zw
        else:
            d_in, ld_in = new(B, E * pe[l - 1], **f32), E * pe[l - 1]
        ws_ = [experts[e][l][0] for e in range(E)]
        gemm_grouped(False, True, B, n_in, n, [fptr(dz, e * pe[l]) for e in range(E)], ld_dz,
                     [w.data_ptr() for w in ws_], ws_[0].stride(0), [fptr(d_in, e * pe[l - 1]) for e in range(E)],
                     ld_in, st, C_mask=[fptr(inp, e * pe[l - 1]) for e in range(E)], ldmask=E * pe[l - 1],
                     mask_scale=scale)
        dz, ld_dz = d_in, ld_in
    # layer 0 of every expert and the K gates: one weight-gradient product, one data-gradient GEMM
    dWs, dbs = wgrad(sh.zw, w4, dZ0, sh.zw, s["x"], w4)
    n0, r0 = sh.eu[0], E * pe[0]
    dW0 = dWs[:r0].view(E, pe[0], w4)[:, :n0, :width].contiguous()   # one cut for all experts, one for all gates
    db0 = dbs[:r0].view(E, pe[0])[:, :n0].contiguous()
    dWg = dWs[r0:r0 + K * E, :width].contiguous().view(K, E, width)
    dbg = dbs[r0:r0 + K * E].view(K, E)
    for e in range(E):
        expert_grads[e][0] = (dW0[e], db0[e])
    gate_grads = [(dWg[k], dbg[k]) for k in range(K)]
    dx = None
    if need_dx:
        dx = torch.empty(B, width, **f32)
        gemm(False, True, B, width, sh.zw, dZ0, sh.zw, wst, wst.stride(0), dx, split=1)
    return dx, expert_grads, gate_grads, tower_grads


class _MmoeFn(torch.autograd.Function):
    """rankops.mmoe with autograd: rk_mmoe_forward_train without dropout, mmoe_backward.  Inputs after the
    fixed arguments: x, then every weight and bias of `layout` flattened (None for an absent bias)."""

    @staticmethod
    def forward(ctx, sh, launch, x, *flat):
        s = launch()
        ctx.sh, ctx.s, ctx.flat, ctx.B = sh, s, flat, x.shape[0]
        B, K, H, E = x.shape[0], sh.K, sh.H, sh.E
        mixed = s["mixed"].view(B, K, p4(H))[:, :, :H]
        outs = (mixed, s["gate_probs"]) + ((s["logits"], s["probs"]) if sh.heads else ())
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None, not as zeros
        return outs

    @staticmethod
    def backward(ctx, d_mixed, d_gates, d_logits=None, d_probs=None):
        sh, s, flat, B = ctx.sh, ctx.s, ctx.flat, ctx.B
        if d_gates is not None:
            raise NotImplementedError("rankops.mmoe: a gradient flowing into gate_probs is not supported "
                                      "(differentiate mixed, logits or probs)")
        experts, gates, towers, wst = s["weights"]
        dev = s["x"].device
        if B == 0:
            return (None, None, torch.zeros(0, sh.width, device=dev)) + tuple(
                None if t is None else torch.zeros_like(t) for t in flat)
        like = lambda g, shape: None if g is None else g.to(torch.float32).reshape(shape).contiguous()
        dx, eg, gg, tg = mmoe_backward(sh, B, s, wst, experts, gates, towers, 0.0, like(d_mixed, (B, sh.K, sh.H)),
                                       like(d_logits, (B, sh.K)), like(d_probs, (B, sh.K)), ctx.needs_input_grad[2],
                                       dev)
        out = []
        for e in range(sh.E):
            for l in range(len(sh.eu)):
                out += list(eg[e][l])
        for k in range(sh.K):
            out += list(gg[k])
        if towers is not None:
            for k in range(sh.K):
                for l in range(len(sh.tu)):
                    out += list(tg[k][0][l])
                out += list(tg[k][1])
        grads = [None if t is None else g.reshape(t.shape) for t, g in zip(flat, out)]
        return (None, None, dx, *grads)


def _mmoe_wants_grad(x, experts, gates, towers):
    ts = [x] + [t for layers in experts for wb in layers for t in wb] + [t for wb in gates for t in wb]
    if towers is not None:
        ts += [t for hidden, out in towers for wb in list(hidden) + [out] for t in wb]
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def mmoe(x: torch.Tensor, experts, gates, towers=None):
    """Multi-gate mixture of experts on rows x [B, width] (float32, unit column stride, any row stride
    >= width), in one launch (rk_mmoe_forward):

        f_e = experts[e](x)                  experts: E lists of (W, b) — Linear + ReLU each, b may be None
        g_k = softmax_e(x W_k^T + b_k)       gates: K (W [E, width], b or None)
        m_k = sum_e g_k[e] f_e
        logit_k = towers[k](m_k)             towers: K (hidden [(W, b)…], (w_out [1, ·], b_out)), hidden layers
                                             Linear + ReLU

    Returns (mixed [B, K, H], gate_probs [B, K, E]); with towers also (logits [B, K], probs [B, K]).
    Differentiable whenever x or any weight or bias requires grad (rk_mmoe_forward_train without dropout
    and the grouped backward, DESIGN.md §4d "Training"): gradients for x, every expert, gate and tower
    (W, b) and the output layers, from the incoming gradients of mixed, logits and probs.  A gradient
    flowing into gate_probs raises NotImplementedError.  With nothing requiring grad the call is the eval
    launch, bit for bit."""
    as_f32(x, "x")
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError(f"rankops.mmoe: x must be [B, width] with unit column stride, got {tuple(x.shape)}")
    B, width = x.shape
    dev = x.device
    E, K = len(experts), len(gates)
    if E == 0 or K == 0:
        raise ValueError("rankops.mmoe: at least one expert and one gate")
    stacks, H = [], None
    for e, layers in enumerate(experts):
        if len(layers) == 0:
            raise ValueError(f"rankops.mmoe: expert {e} has no layer")
        st, h = _mmoe_stack(layers, width, f"expert {e}", B > 0)
        if H is not None and h != H:
            raise ValueError(f"rankops.mmoe: expert {e} ends {h} wide, expert 0 {H}")
        stacks.append(st)
        H = h
    for k, (w, b) in enumerate(gates):
        as_f32(w, f"gate {k} weight")
        if tuple(w.shape) != (E, width) or (b is not None and tuple(as_f32(b, f"gate {k} bias").shape) != (E,)):
            raise ValueError(f"rankops.mmoe: gate {k} must be (W [{E}, {width}], b [{E}] or None)")
    gate_image = pack_mlp_weight(torch.cat([w.detach() for w, _ in gates], 0)) if B > 0 else None
    gate_bias = None
    if B > 0 and any(b is not None for _, b in gates):
        gate_bias = torch.cat([b.detach() if b is not None else torch.zeros(E, device=dev) for _, b in gates], 0)
    tstacks = heads = None
    if towers is not None:
        if len(towers) != K:
            raise ValueError(f"rankops.mmoe: {K} gates need {K} towers, got {len(towers)}")
        tstacks, heads = [], []
        for k, (hidden, (w_out, b_out)) in enumerate(towers):
            st, last = _mmoe_stack(hidden, H, f"tower {k}", B > 0)
            as_f32(w_out, f"tower {k} output weight")
            as_f32(b_out, f"tower {k} output bias")
            if w_out.numel() != last or b_out.numel() != 1:
                raise ValueError(f"rankops.mmoe: tower {k} output must be (w [1, {last}], b [1])")
            tstacks.append(st)
            heads.append((w_out.detach().reshape(-1).contiguous(), b_out.detach().reshape(1)))
    if _mmoe_wants_grad(x, experts, gates, towers):
        eu = [w.shape[0] for w, _ in experts[0]]
        tu = [w.shape[0] for w, _ in towers[0][0]] if towers is not None else []
        if any([w.shape[0] for w, _ in layers] != eu for layers in experts) or (
                towers is not None and any([w.shape[0] for w, _ in hidden] != tu for hidden, _ in towers)):
            raise ValueError("rankops.mmoe: with autograd all experts (towers) must have the same widths")
        sh = MmoeShape(width, E, K, eu, tu, towers is not None)
        dexp = [[(w.detach(), b) for w, b in layers] for layers in experts]
        dgat = [(w.detach(), b) for w, b in gates]
        dtow = None if towers is None else [([(w.detach(), b) for w, b in hidden], (wo.detach().reshape(-1), bo))
                                            for hidden, (wo, bo) in towers]
        wst = mmoe_stacked_weight(sh, dexp, dgat) if B > 0 else None  # (an empty batch launches nothing)
        segs = [dense_segment(x.detach(), min(128, width - c), c, c) for c in range(0, width, 128)]

        def launch():
            s = mmoe_forward_train(segs, sh, B, stacks, gate_image, gate_bias, tstacks, heads, dev, 0.0, 0, None)
            s["weights"] = (dexp, dgat, dtow, wst)
            return s
        flat = [t for layers in experts for wb in layers for t in wb] + [t for wb in gates for t in wb]
        if towers is not None:
            flat += [t for hidden, out in towers for wb in list(hidden) + [out] for t in wb]
        return _MmoeFn.apply(sh, launch, x, *flat)
    mixed = torch.empty(B, K, H, device=dev, dtype=torch.float32)
    gate_probs = torch.empty(B, K, E, device=dev, dtype=torch.float32)
    logits = probs = None
    if towers is not None:
        logits = torch.empty(B, K, device=dev, dtype=torch.float32)
        probs = torch.empty(B, K, device=dev, dtype=torch.float32)
    if B > 0:
        # (a segment holds at most 255 columns: the kernel's column map is one byte per column)
        segs = [dense_segment(x, min(128, width - c), c, c) for c in range(0, width, 128)]
        args, _keep = mmoe_forward_args(segs, width, B, stacks, gate_image, gate_bias, K,
                                        tstacks, heads, dev, logits=logits, probs=probs, mixed=mixed,
                                        gate_probs=gate_probs)
        args[-1] = _lib.raw_stream(dev)
        check(_lib.load().rk_mmoe_forward(*args), "rk_mmoe_forward")
    return (mixed, gate_probs) if towers is None else (mixed, gate_probs, logits, probs)


# ---------------------------------------------------------------- PLE (rk_ple_forward)

# argument slots of rk_ple_forward patched per call (ple_forward_args)
PLE_LOGITS_SLOT, PLE_PROBS_SLOT = 15, 16

_PLE_TABLES = {}


def ple_table(entries, device):
    """The device table of rk_ple_forward: [(weight image or head weight, bias or None)…] in the order of
    include/rankops.h, as a uint8 tensor holding rk_mmoe_layer structs.  Memoized on its bytes (the
    addresses): a forward rebuilt over the same images reuses the table, so that building one inside a
    hipGraph capture copies nothing."""
    arr = (_lib.MmoeLayer * len(entries))()
    for d, (w, b) in zip(arr, entries):
        d.w, d.bias = w.data_ptr(), ptr(b)
    raw = bytes(arr)
    key = (str(device), raw)
    hit = _PLE_TABLES.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("rankops.ple: the layer table of these weights is not on the device yet and cannot be "
                               "uploaded inside a hipGraph capture; run the forward once before capturing")
        hit = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
        if len(_PLE_TABLES) >= 64:
            _PLE_TABLES.pop(next(iter(_PLE_TABLES)))
        _PLE_TABLES[key] = hit
    return hit


def ple_forward_args(segs, width, batch, num_levels, num_tasks, num_specific, num_shared, expert_units, tower_units,
                     entries, has_heads, device, *, logits=None, probs=None, reps=None, gates=None):
    """The rk_ple_forward argument list (the stream last, None) and what it points into.  entries: the
    layer table's (image, bias) pairs in the header's order (experts level-major, gates, towers, heads);
    reps / gates: lists of L tensors (or None) for the per-level outputs.  logits [15], probs [16] and
    the stream [-1] are the per-call slots of a cached forward."""
    _lib.ensure_device(device)
    arr = _as_seg_array(segs)
    eu = (ctypes.c_int32 * max(1, len(expert_units)))(*expert_units)
    tu = (ctypes.c_int32 * max(1, len(tower_units)))(*tower_units)
    table = ple_table(entries, device)

    def ptrs(ts):
        return None if ts is None else (ctypes.c_void_p * num_levels)(*[ptr(t) for t in ts])
    rp, gp = ptrs(reps), ptrs(gates)
    args = [arr, len(arr), width, batch, num_levels, num_tasks, num_specific, num_shared, eu, len(expert_units),
            tu if tower_units else None, len(tower_units), int(bool(has_heads)), table.data_ptr(), len(entries),
            ptr(logits), ptr(probs), rp, gp, None]
    return args, (arr, eu, tu, table, rp, gp, entries)


def _ple_pair(wb, n, k, what):
    w, b = wb
    as_f32(w, f"{what} weight")
    if w.dim() != 2 or w.stride(1) != 1 or (n is not None and w.shape[0] != n) or w.shape[1] != k:
        raise ValueError(f"rankops.ple: {what} weight must be [{'n' if n is None else n}, {k}] with unit column "
                         f"stride, got {tuple(w.shape)}")
    if b is not None and (as_f32(b, f"{what} bias").dim() != 1 or b.shape[0] != w.shape[0] or not b.is_contiguous()):
        raise ValueError(f"rankops.ple: {what} bias must be a contiguous [{w.shape[0]}] tensor")
    return w.detach(), (b.detach() if b is not None else None)


def ple(x: torch.Tensor, levels, towers=None, return_levels=False):
    """Progressive layered extraction on rows x [B, width] (float32, unit column stride, any row stride
    >= width), in one launch (rk_ple_forward).  levels[j] = (specific, shared, gates, shared_gate):

        specific: K lists (one per task) of ms experts, shared: mc experts; an expert is a list of (W, b),
                  Linear + ReLU each, b may be None; level 0 reads x, later levels the H-wide representations
        gates: K (W [ms + mc, in], b or None); shared_gate: (W [K ms + mc, in], b or None), None at the last level

    (the definition: rankops.PLE).  towers: K (hidden [(W, b)…], (w_out [1, ·], b_out)) or None.
    Returns (logits [B, K], probs [B, K]) with towers, else the last level's (representations [B, K, H],
    gates [B, K, ms + mc]).  return_levels=True appends (with towers) or returns instead (without) the list
    over the levels of (representations [B, K + 1, H] — the tasks', then the shared one; [B, K, H] at the
    last level —, task gates [B, K, ms + mc], shared gate [B, K ms + mc] or None).
    Differentiable whenever grad is enabled and x or any weight or bias requires grad (rk_ple_forward_train
    without dropout and ple_backward, DESIGN.md §4e "Training"): gradients for x and every (W, b) from the
    incoming gradients of logits, probs and the last level's representations.  A gradient flowing into a
    gate output or into a lower level's representations raises NotImplementedError.  With nothing requiring
    grad the call is the eval launch, bit for bit."""
    as_f32(x, "x")
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError(f"rankops.ple: x must be [B, width] with unit column stride, got {tuple(x.shape)}")
    B, width = x.shape
    dev = x.device
    L = len(levels)
    if L == 0:
        raise ValueError("rankops.ple: at least one level")
    K = len(levels[0][2])
    ms = len(levels[0][0][0]) if K and len(levels[0][0]) else 0
    mc = len(levels[0][1])
    if K == 0 or mc == 0:
        raise ValueError("rankops.ple: at least one task gate and one shared expert per level")
    eu = [w.shape[0] for w, _ in levels[0][1][0]]
    if len(eu) == 0:
        raise ValueError("rankops.ple: an expert has no layer")
    H, NE = eu[-1], K * ms + mc
    experts, gate_entries = [], []
    for j, (specific, shared, gates, shared_gate) in enumerate(levels):
        k_in = width if j == 0 else H
        if len(specific) != K or any(len(s) != ms for s in specific) or len(shared) != mc or len(gates) != K:
            raise ValueError(f"rankops.ple: level {j} must hold {K} x {ms} task experts, {mc} shared experts and {K} gates")
        if (shared_gate is None) != (j == L - 1):
            raise ValueError("rankops.ple: every level but the last has a shared gate, the last has none")
        stacks = [e for s in specific for e in s] + list(shared)
        for s, layers in enumerate(stacks):
            if len(layers) != len(eu):
                raise ValueError(f"rankops.ple: level {j} expert {s} must have {len(eu)} layers")
            k = k_in
            for l, wb in enumerate(layers):
                experts.append(_ple_pair(wb, eu[l], k, f"level {j} expert {s} layer {l}"))
                k = eu[l]
        for q, wb in enumerate(gates):
            gate_entries.append(_ple_pair(wb, ms + mc, k_in, f"level {j} gate {q}"))
        gate_entries.append(_ple_pair(shared_gate, NE, k_in, f"level {j} shared gate") if shared_gate is not None
                            else None)
    tu, tower_entries, heads = [], [], []
    if towers is not None:
        if len(towers) != K:
            raise ValueError(f"rankops.ple: {K} gates need {K} towers, got {len(towers)}")
        tu = [w.shape[0] for w, _ in towers[0][0]]
        for k, (hidden, (w_out, b_out)) in enumerate(towers):
            if len(hidden) != len(tu):
                raise ValueError("rankops.ple: every tower must have the same layers")
            kin = H
            for l, wb in enumerate(hidden):
                tower_entries.append(_ple_pair(wb, tu[l], kin, f"tower {k} layer {l}"))
                kin = tu[l]
            as_f32(w_out, f"tower {k} output weight")
            as_f32(b_out, f"tower {k} output bias")
            if w_out.numel() != kin or b_out.numel() != 1:
                raise ValueError(f"rankops.ple: tower {k} output must be (w [1, {kin}], b [1])")
            heads.append((w_out.detach().reshape(-1).contiguous(), b_out.detach().reshape(1)))
    from . import common
    if not common.ple_fits(width, (width + 127) // 128, L, K, ms, mc, eu, tu):
        raise RuntimeError("rankops.ple: configuration outside rk_ple_forward's envelope (common.ple_fits)")
    flat = _ple_flat(levels, towers)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [x] + flat):
        return _ple_autograd(x, flat, PleShape(width, L, K, ms, mc, eu, tu, towers is not None), experts, gate_entries,
                             tower_entries, heads, return_levels)
    want = return_levels or towers is None
    GT = ms + mc
    reps = [torch.empty(B, K + (j < L - 1), H, device=dev, dtype=torch.float32) if want and (return_levels or j == L - 1)
            else None for j in range(L)]
    gate_out = [torch.empty(B, K * GT + (NE if j < L - 1 else 0), device=dev, dtype=torch.float32)
                if want and (return_levels or j == L - 1) else None for j in range(L)]
    logits = probs = None
    if towers is not None:
        logits = torch.empty(B, K, device=dev, dtype=torch.float32)
        probs = torch.empty(B, K, device=dev, dtype=torch.float32)
    if B > 0:
        stream = _lib.raw_stream(dev)
        packed = [wb for wb in experts + gate_entries + tower_entries if wb is not None]
        images = [mlp_image(w.shape[0], w.shape[1], dev) for w, _ in packed]
        pack_mlp_weights([(w, img) for (w, _), img in zip(packed, images)], stream)  # every image in one launch
        it = iter(images)
        zero = images[0]
        entries = [(next(it), wb[1]) if wb is not None else (zero, None) for wb in experts + gate_entries + tower_entries]
        entries += heads
        segs = [dense_segment(x, min(128, width - c), c, c) for c in range(0, width, 128)]
        args, _keep = ple_forward_args(segs, width, B, L, K, ms, mc, eu, tu, entries, towers is not None, dev,
                                       logits=logits, probs=probs, reps=reps if want else None,
                                       gates=gate_out if want else None)
        args[-1] = stream
        check(_lib.load().rk_ple_forward(*args), "rk_ple_forward")

    def split(j):
        g = gate_out[j]
        return (reps[j], g[:, :K * GT].view(B, K, GT), g[:, K * GT:] if j < L - 1 else None)
    if towers is None:
        return [split(j) for j in range(L)] if return_levels else split(L - 1)[:2]
    return (logits, probs, [split(j) for j in range(L)]) if return_levels else (logits, probs)


# ---------------------------------------------------------------- PLE training ("Training")

class PleShape:
    """Widths of one PLE (L levels of K x ms task stacks and mc shared ones, units eu; K towers of units tu)
    and the column layout of every level's dZ0, the buffer that holds the gradients of all the level's
    first-layer pre-activations and gate logits side by side (every block on the 4 grid, zeros between):

        level 0     [dz_{0,0} … dz_{NE-1,0} | dgl_0 … dgl_{K-1} | dgl_K]      every stack and gate reads x
        level j>=1  K task blocks [dz_{s,0} of the task's ms stacks | dgl_q], then the shared block
                    [dz_{s,0} of the mc shared stacks | dgl_K]                 owner q reads x_q^{j-1}

    (dgl_K, the shared gate's, is absent at the last level)."""

    def __init__(self, width, L, K, ms, mc, eu, tu, heads: bool):
        self.width, self.L, self.K, self.ms, self.mc = width, L, K, ms, mc
        self.eu, self.tu, self.heads = tuple(eu), tuple(tu), heads
        self.H, self.NE, self.GT = self.eu[-1], K * ms + mc, ms + mc

    def nq(self, j):
        return self.K + (j < self.L - 1)

    def gcols(self, j):
        return self.K * self.GT + (self.NE if j < self.L - 1 else 0)

    def layout(self, j):
        """(columns of dZ0^j, stack offsets [NE], gate offsets [nq], task block width, shared block width)."""
        K, ms, mc, NE, pe0, pg = self.K, self.ms, self.mc, self.NE, p4(self.eu[0]), p4(self.GT)
        ps = p4(NE) if j < self.L - 1 else 0
        if j == 0:
            soff = [s * pe0 for s in range(NE)]
            goff = [NE * pe0 + q * pg for q in range(self.nq(0))]
            return NE * pe0 + K * pg + ps, soff, goff, 0, 0
        bw_t, bw_s = ms * pe0 + pg, mc * pe0 + ps
        soff = [q * bw_t + i * pe0 for q in range(K) for i in range(ms)] + [K * bw_t + i * pe0 for i in range(mc)]
        goff = [q * bw_t + ms * pe0 for q in range(K)] + ([K * bw_t + mc * pe0] if ps else [])
        return K * bw_t + bw_s, soff, goff, bw_t, bw_s

    def padded(self):
        """dZ0 has pad columns that no kernel writes: those behind a first layer off the 4 grid that
        rk_gemm_grouped fills (rk_ple_mix_backward writes zeros into the pad columns of everything it
        stores, the gates' included).  It is then zero-filled: the stacked data gradient reads them."""
        return bool(self.eu[0] % 4 and len(self.eu) > 1)


def _ple_flat(levels, towers):
    """Every weight and bias of rankops.ple's arguments in a fixed order (None for an absent bias): per
    level the stacks' layers (stack-major), the K gates, the shared gate; then the towers."""
    flat = []
    for specific, shared, gates, shared_gate in levels:
        flat += [t for task in specific for layers in task for wb in layers for t in wb]
        flat += [t for layers in shared for wb in layers for t in wb]
        flat += [t for wb in gates for t in wb]
        if shared_gate is not None:
            flat += list(shared_gate)
    if towers is not None:
        flat += [t for hidden, out in towers for wb in list(hidden) + [out] for t in wb]
    return flat


def ple_level_lists(sh: PleShape, experts, gate_entries):
    """[(stacks [NE][De] of (W, b), gates [nq] of (W, b))…] from the layer table's flat order."""
    De, NE, K = len(sh.eu), sh.NE, sh.K
    return [([[experts[(j * NE + s) * De + l] for l in range(De)] for s in range(NE)],
             [gate_entries[j * (K + 1) + q] for q in range(sh.nq(j))]) for j in range(sh.L)]


def ple_stacked_weights(sh: PleShape, levels):
    """The stacked first-layer / gate weights behind dZ0 (PleShape), rows and columns on the 4 grid with
    zeros between: level 0 one [zw, p4(width)] matrix; level j >= 1 (task owners [K, bw_t, p4(H)], shared owner
    [bw_s, p4(H)]).  A fixed number of launches per level whatever K, ms and mc."""
    K, ms, mc, pe0, n0 = sh.K, sh.ms, sh.mc, p4(sh.eu[0]), sh.eu[0]
    pad = torch.nn.functional.pad

    def block(ws, n, k_in):  # count weights [n, k_in] -> [count, p4(n), p4(k_in)]
        # (padded even when on the grid: whether ms + mc or K ms + mc is must not change the launch list)
        return pad(torch.stack(ws, 0), (0, p4(k_in) - k_in, 0, p4(n) - n))
    out = []
    for j, (stacks, gates) in enumerate(levels):
        k_in = sh.width if j == 0 else sh.H
        kp = p4(k_in)
        first = [layers[0][0] for layers in stacks]
        tg = block([w for w, _ in gates[:K]], sh.GT, k_in)
        shared = [block(first[K * ms:], n0, k_in).view(mc * pe0, kp)]
        if len(gates) > K:
            shared.append(block([gates[K][0]], sh.NE, k_in)[0])
        task = block(first[:K * ms], n0, k_in) if ms else None
        if j == 0:
            parts = ([task.view(K * ms * pe0, kp)] if ms else []) + [shared[0], tg.view(K * p4(sh.GT), kp)] + shared[1:]
            out.append(torch.cat(parts, 0))
        else:
            wt = torch.cat([task.view(K, ms * pe0, kp), tg], 1) if ms else tg.contiguous()
            out.append((wt, torch.cat(shared, 0) if len(shared) > 1 else shared[0]))
    return out


def ple_forward_train(segs, sh: PleShape, B, entries, device, p, seed, slot):
    """rk_ple_forward_train: one launch; returns the saved buffers (include/rankops.h) as a dict."""
    new = torch.empty  # (the kernel writes the pad columns)
    f32 = dict(device=device, dtype=torch.float32)
    L, K, NE, pm = sh.L, sh.K, sh.NE, p4(sh.H)
    s = dict(x=new(B, p4(sh.width), **f32), eacts=[[new(B, NE * p4(n), **f32) for n in sh.eu] for _ in range(L)],
             tacts=[new(B, K * p4(n), **f32) for n in sh.tu], reps=[new(B, sh.nq(j) * pm, **f32) for j in range(L)],
             gates=[new(B, sh.gcols(j), **f32) for j in range(L)], logits=None, probs=None)
    if sh.heads:
        s["logits"], s["probs"] = new(B, K, **f32), new(B, K, **f32)
    if B == 0:
        return s
    args, keep = ple_forward_args(segs, sh.width, B, L, K, sh.ms, sh.mc, sh.eu, sh.tu, entries, sh.heads, device)
    ea = _ptrs([t.data_ptr() for lv in s["eacts"] for t in lv])
    ta = _ptrs([t.data_ptr() for t in s["tacts"]]) if sh.tu else None
    call = args[:15] + [float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(slot), s["x"].data_ptr(), ea, ta, ptr(s["logits"]),
                        ptr(s["probs"]), _ptrs([t.data_ptr() for t in s["reps"]]),
                        _ptrs([t.data_ptr() for t in s["gates"]]), _lib.raw_stream(device)]
    check(_lib.load().rk_ple_forward_train(*call), "rk_ple_forward_train")
    return s


def ple_mix_backward(B, K, ms, mc, has_shared_mix, H, dm, ld_dm, pitch_dm, f, ld_f, pitch_f, gates, ld_gates, mask_scale,
                     dgl, ld_dgl, gate_offsets, dz, ld_dz, stack_offsets, pitch_dz, stream):
    """rk_ple_mix_backward; dm, f, gates, dgl, dz are device addresses or tensors, the offsets lists of ints."""
    a = [t.data_ptr() if isinstance(t, torch.Tensor) else t for t in (dm, f, gates, dgl, dz)]
    go = (ctypes.c_int32 * max(1, len(gate_offsets)))(*gate_offsets)
    so = (ctypes.c_int32 * max(1, len(stack_offsets)))(*stack_offsets)
    check(_lib.load().rk_ple_mix_backward(B, K, ms, mc, int(bool(has_shared_mix)), H, a[0], ld_dm, pitch_dm, a[1], ld_f,
                                          pitch_f, a[2], ld_gates, mask_scale, a[3], ld_dgl, go, a[4], ld_dz, so,
                                          pitch_dz, stream), "rk_ple_mix_backward")


def ple_backward(sh: PleShape, B, s, wst, levels, towers, p, d_reps, d_logits, d_probs, need_dx, device):
    """The PLE backward from the buffers of ple_forward_train (s), the stacked first-layer / gate weights
    (wst, ple_stacked_weights) and the plain weights (levels: ple_level_lists' form; towers: K (hidden,
    (w, b)) or None).  d_reps [B, K, H] (into the last level's representations), d_logits, d_probs [B, K]:
    the incoming gradients, each may be None.  Returns (dx [B, width] or None, per level (stack grads
    [[(dW, db)…]…], gate grads [(dW, db)…]), tower grads or None); a db is returned for every layer.
    Heads and towers as MMoE's (mtl_tower_backward); then per level, going down: rk_ple_mix_backward,
    per expert layer above the first the grouped pair over the level's stacks in chunks of 16, and
    layer 0 with the gates through dZ0 (PleShape) — level 0 as one rk_gemm_wgrad and one rk_gemm against
    x, a later level as one rk_gemm_wgrad_grouped + rk_gemm_grouped over the K task owners and one
    rk_gemm_wgrad + rk_gemm for the shared owner, which write the gradient of the level below's
    representations.  The launches depend on L, De, Dt and ceil(NE / 16) only; no float atomics,
    fixed-order sums."""
    L, K, ms, mc, NE, GT, H, width = sh.L, sh.K, sh.ms, sh.mc, sh.NE, sh.GT, sh.H, sh.width
    De = len(sh.eu)
    pe, pm, w4, n0 = [p4(n) for n in sh.eu], p4(H), p4(width), sh.eu[0]
    pe0, pg = pe[0], p4(GT)
    f32 = dict(device=device, dtype=torch.float32)
    # Pad columns: as in mmoe_backward (the mix kernel writes zeros into its own, rk_gemm_grouped leaves those
    # of its outputs unwritten, which only reach cut-away rows of padded weight gradients; dZ0's are read by
    # the stacked data gradient, so a dZ0 that has any is zero-filled).
    new = torch.empty
    st = _lib.raw_stream(device)
    scale = 1.0 / (1.0 - p)
    dR, tower_grads = mtl_tower_backward(K, H, sh.tu, B, s["tacts"], s["reps"][L - 1], s["probs"], towers, scale, d_reps,
                                         d_logits, d_probs, device, st)
    level_grads = [None] * L
    dx = None
    for j in range(L - 1, -1, -1):
        stacks, gates = levels[j]
        nq = sh.nq(j)
        zw, soff, goff, bw_t, bw_s = sh.layout(j)
        dZ0 = (torch.zeros if sh.padded() else new)(B, zw, **f32)
        if De == 1:
            dz, ld_dz, zoff = dZ0, zw, soff
        else:
            dz, ld_dz, zoff = new(B, NE * pe[-1], **f32), NE * pe[-1], [i * pe[-1] for i in range(NE)]
        ple_mix_backward(B, K, ms, mc, nq > K, H, dR, nq * pm, pm, s["eacts"][j][-1], NE * pe[-1], pe[-1], s["gates"][j],
                         sh.gcols(j), scale, dZ0, zw, goff, dz, ld_dz, zoff, pe[-1], st)
        sg = [[None] * De for _ in range(NE)]
        for l in range(De - 1, 0, -1):
            n, n_in = sh.eu[l], sh.eu[l - 1]
            inp, ld_inp = s["eacts"][j][l - 1], NE * pe[l - 1]
            dW, db = new(NE, pe[l], pe[l - 1], **f32), new(NE, pe[l], **f32)
            if l == 1:
                d_in, ld_in, ioff = dZ0, zw, soff
            else:
                d_in, ld_in, ioff = new(B, ld_inp, **f32), ld_inp, [i * pe[l - 1] for i in range(NE)]
            for c0 in range(0, NE, 16):  # (rk_gemm_grouped takes 16 groups)
                ss = range(c0, min(NE, c0 + 16))
                A = [fptr(dz, zoff[i]) for i in ss]
                X = [fptr(inp, i * pe[l - 1]) for i in ss]
                gemm_wgrad_grouped(pe[l], pe[l - 1], B, A, ld_dz, X, ld_inp, [dW[i].data_ptr() for i in ss], pe[l - 1],
                                   [db[i].data_ptr() for i in ss], device, st)
                ws_ = [stacks[i][l][0] for i in ss]
                gemm_grouped(False, True, B, n_in, n, A, ld_dz, [w.data_ptr() for w in ws_], ws_[0].stride(0),
                             [fptr(d_in, ioff[i]) for i in ss], ld_in, st, C_mask=X, ldmask=ld_inp, mask_scale=scale)
            dW, db = dW[:, :n, :n_in].contiguous(), db[:, :n].contiguous()  # (no launch unless padded)
            for i in range(NE):
                sg[i][l] = (dW[i], db[i])
            dz, ld_dz, zoff = d_in, ld_in, ioff
        if j == 0:
            # every stack and gate reads x: one weight-gradient product, one data-gradient GEMM
            dWs, dbs = _wgrad(B, zw, w4, dZ0, zw, s["x"], w4, device, st)
            r0 = NE * pe0
            dW0 = dWs[:r0].view(NE, pe0, w4)[:, :n0, :width].contiguous()
            db0 = dbs[:r0].view(NE, pe0)[:, :n0].contiguous()
            # (the gates' cuts are clones: a copy whether or not ms + mc is on the grid, as above)
            dWg = dWs[r0:r0 + K * pg].view(K, pg, w4)[:, :GT, :width].clone()
            dbg = dbs[r0:r0 + K * pg].view(K, pg)[:, :GT].clone()
            gg = [(dWg[q], dbg[q]) for q in range(K)]
            if nq > K:
                gg.append((dWs[goff[K]:goff[K] + NE, :width].contiguous(), dbs[goff[K]:goff[K] + NE]))
            if need_dx:
                dx = new(B, width, **f32)
                gemm(False, True, B, width, zw, dZ0, zw, wst[0], wst[0].stride(0), dx, split=1)
        else:
            # owner q reads x_q^{j-1}: the K task owners grouped, the shared owner on its own
            wt, wsh = wst[j]
            prev, ld_prev = s["reps"][j - 1], (K + 1) * pm
            dWt, dbt = new(K, bw_t, pm, **f32), new(K, bw_t, **f32)
            A = [fptr(dZ0, q * bw_t) for q in range(K)]
            gemm_wgrad_grouped(bw_t, pm, B, A, zw, [fptr(prev, q * pm) for q in range(K)], ld_prev,
                               [dWt[q].data_ptr() for q in range(K)], pm, [dbt[q].data_ptr() for q in range(K)], device, st)
            dZs, prev_s = dZ0[:, K * bw_t:], prev[:, K * pm:]
            dWs, dbs = _wgrad(B, bw_s, pm, dZs, zw, prev_s, ld_prev, device, st)
            dR = new(B, ld_prev, **f32)  # (its pad columns come out zero: the stacked weights' are)
            gemm_grouped(False, True, B, pm, bw_t, A, zw, [wt[q].data_ptr() for q in range(K)], pm,
                         [fptr(dR, q * pm) for q in range(K)], ld_prev, st)
            gemm(False, True, B, pm, bw_s, dZs, zw, wsh, pm, dR[:, K * pm:], ld_prev, split=1)
            r0 = ms * pe0
            dW0t = dWt[:, :r0, :H].clone().view(K * ms, pe0, H)[:, :n0].contiguous()
            db0t = dbt[:, :r0].clone().view(K * ms, pe0)[:, :n0].contiguous()
            dW0s = dWs[:mc * pe0].view(mc, pe0, pm)[:, :n0, :H].contiguous()
            db0s = dbs[:mc * pe0].view(mc, pe0)[:, :n0].contiguous()
            dW0, db0 = list(dW0t) + list(dW0s), list(db0t) + list(db0s)
            dWg, dbg = dWt[:, r0:r0 + GT, :H].clone(), dbt[:, r0:r0 + GT].clone()
            gg = [(dWg[q], dbg[q]) for q in range(K)]
            if nq > K:
                gg.append((dWs[mc * pe0:mc * pe0 + NE, :H].contiguous(), dbs[mc * pe0:mc * pe0 + NE]))
        for i in range(NE):
            sg[i][0] = (dW0[i], db0[i])
        level_grads[j] = (sg, gg)
    return dx, level_grads, tower_grads


def ple_flat_grads(sh: PleShape, level_grads, tower_grads):
    """ple_backward's gradients in _ple_flat's order (a (dW, db) per layer, bias-free ones included)."""
    out = []
    for sg, gg in level_grads:
        out += [t for layers in sg for wb in layers for t in wb]
        out += [t for wb in gg for t in wb]
    if tower_grads is not None:
        for hidden, head in tower_grads:
            out += [t for wb in hidden for t in wb] + list(head)
    return out


class _PleFn(torch.autograd.Function):
    """rankops.ple with autograd: rk_ple_forward_train without dropout, ple_backward.  Inputs after the
    fixed arguments: x, then every weight and bias in _ple_flat's order (None for an absent bias).
    Outputs: per level (representations, gates), then logits and probs with towers."""

    @staticmethod
    def forward(ctx, sh, launch, x, *flat):
        s = launch()
        ctx.sh, ctx.s, ctx.flat, ctx.B = sh, s, flat, x.shape[0]
        B, pm = x.shape[0], p4(sh.H)
        outs = []
        for j in range(sh.L):
            outs += [s["reps"][j].view(B, sh.nq(j), pm)[:, :, :sh.H], s["gates"][j]]
        if sh.heads:
            outs += [s["logits"], s["probs"]]
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None, not as zeros
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        sh, s, flat, B = ctx.sh, ctx.s, ctx.flat, ctx.B
        L = sh.L
        if any(g is not None for j in range(L) for g in (grads[2 * j + 1],) + ((grads[2 * j],) if j < L - 1 else ())):
            raise NotImplementedError("rankops.ple: a gradient flowing into a gate output or a lower level's "
                                      "representations is not supported (differentiate logits, probs or the last "
                                      "level's representations)")
        d_reps = grads[2 * (L - 1)]
        d_logits, d_probs = (grads[2 * L], grads[2 * L + 1]) if sh.heads else (None, None)
        levels, towers, wst = s["weights"]
        dev = s["x"].device
        if B == 0:
            return (None, None, torch.zeros(0, sh.width, device=dev)) + tuple(
                None if t is None else torch.zeros_like(t) for t in flat)
        like = lambda g, shape: None if g is None else g.to(torch.float32).reshape(shape).contiguous()
        dx, lg, tg = ple_backward(sh, B, s, wst, levels, towers, 0.0, like(d_reps, (B, sh.K, sh.H)),
                                  like(d_logits, (B, sh.K)), like(d_probs, (B, sh.K)), ctx.needs_input_grad[2], dev)
        out = ple_flat_grads(sh, lg, tg)
        return (None, None, dx, *[None if t is None else g.reshape(t.shape) for t, g in zip(flat, out)])


def _ple_autograd(x, flat, sh: PleShape, experts, gate_entries, tower_entries, heads, return_levels):
    """rankops.ple's differentiable path over the checked, detached (W, b) lists of ops.ple."""
    B, dev, L, K, GT = x.shape[0], x.device, sh.L, sh.K, sh.GT
    Dt = len(sh.tu)
    levels = ple_level_lists(sh, experts, gate_entries)
    towers = None
    if sh.heads:
        towers = [(tower_entries[k * Dt:(k + 1) * Dt], heads[k]) for k in range(K)]

    def launch():
        if B == 0:  # (an empty batch launches nothing)
            s = ple_forward_train(None, sh, 0, None, dev, 0.0, 0, None)
            s["weights"] = (levels, towers, None)
            return s
        stream = _lib.raw_stream(dev)
        table = experts + gate_entries + tower_entries
        packed = [wb for wb in table if wb is not None]
        images = [mlp_image(w.shape[0], w.shape[1], dev) for w, _ in packed]
        pack_mlp_weights([(w, img) for (w, _), img in zip(packed, images)], stream)
        it = iter(images)
        entries = [(next(it), wb[1]) if wb is not None else (images[0], None) for wb in table] + heads
        segs = [dense_segment(x.detach(), min(128, sh.width - c), c, c) for c in range(0, sh.width, 128)]
        s = ple_forward_train(segs, sh, B, entries, dev, 0.0, 0, None)
        s["weights"] = (levels, towers, ple_stacked_weights(sh, levels))
        return s
    out = _PleFn.apply(sh, launch, x, *flat)

    def split(j):
        g = out[2 * j + 1]
        return (out[2 * j], g[:, :K * GT].view(B, K, GT), g[:, K * GT:] if j < L - 1 else None)
    if not sh.heads:
        return [split(j) for j in range(L)] if return_levels else split(L - 1)[:2]
    logits, probs = out[2 * L], out[2 * L + 1]
    return (logits, probs, [split(j) for j in range(L)]) if return_levels else (logits, probs)


# ---------------------------------------------------------------- ESMM (rk_esmm_forward)

# argument slots of rk_esmm_forward patched per call (esmm_forward_args)
ESMM_LOGITS_SLOT, ESMM_PROBS_SLOT, ESMM_COND_SLOT = 9, 10, 11


def esmm_forward_args(segs, width, batch, towers, heads, device, *, logits=None, probs=None, cond=None):
    """The rk_esmm_forward argument list (the stream last, None) and the ctypes arrays it points into.
    towers: K stacks of equal depth, each a list of (pack_mlp_weight image, bias or None, n, act); heads: K
    (w [last width], b [1]).  logits [9], probs [10], cond [11] and the stream [-1] are the per-call slots
    of a cached forward."""
    _lib.ensure_device(device)
    arr = _as_seg_array(segs)
    K = len(towers)
    depth = len(towers[0]) if towers else 0
    if any(len(s) != depth for s in towers):
        raise ValueError("rankops.esmm: every tower must have the same number of layers")
    if len(heads) != K:
        raise ValueError(f"rankops.esmm: {K} towers need {K} heads")
    tw = _mmoe_layer_array(towers)
    hw = (ctypes.c_void_p * max(1, K))(*[w.data_ptr() for w, _ in heads])
    hb = (ctypes.c_void_p * max(1, K))(*[b.data_ptr() for _, b in heads])
    args = [arr, len(arr), width, batch, tw, K, depth, hw, hb, ptr(logits), ptr(probs), ptr(cond), None]
    return args, (arr, tw, hw, hb)


class EsmmShape:
    """Widths of one ESMM: the row and K towers of units tu."""

    def __init__(self, width, K, tu):
        self.width, self.K, self.tu = width, K, tuple(tu)


def esmm_stacked_weight(sh: EsmmShape, towers):
    """[W_{0,0}; …; W_{K-1,0}] as one [K p4(n_0), p4(width)] matrix (rows and columns on the 4 grid, zeros
    between): layer 0 of every tower reads the same x, so their data gradient is one GEMM against it and
    their weight gradients one product (as mmoe_stacked_weight)."""
    first = [hidden[0][0].detach() for hidden, _ in towers]
    pad = torch.nn.functional.pad
    n0, cols = sh.tu[0], p4(sh.width) - sh.width
    if n0 % 4 == 0:
        out = torch.cat(first, 0)
        return pad(out, (0, cols)) if cols else out
    return pad(torch.stack(first, 0), (0, cols, 0, p4(n0) - n0)).view(sh.K * p4(n0), p4(sh.width))


def esmm_forward_train(segs, sh: EsmmShape, B, tstacks, heads, device, p, seed, slot):
    """rk_esmm_forward_train: one launch; returns the saved buffers (include/rankops.h) as a dict."""
    f32 = dict(device=device, dtype=torch.float32)
    K = sh.K
    s = dict(x=torch.empty(B, p4(sh.width), **f32), tacts=[torch.empty(B, K * p4(n), **f32) for n in sh.tu],
             logits=torch.empty(B, K, **f32), probs=torch.empty(B, K, **f32), cond=torch.empty(B, K, **f32))
    if B == 0:
        return s
    args, keep = esmm_forward_args(segs, sh.width, B, tstacks, heads, device)
    ta = _ptrs([t.data_ptr() for t in s["tacts"]])
    call = args[:9] + [float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(slot), s["x"].data_ptr(), ta, s["logits"].data_ptr(),
                       s["probs"].data_ptr(), s["cond"].data_ptr(), _lib.raw_stream(device)]
    check(_lib.load().rk_esmm_forward_train(*call), "rk_esmm_forward_train")
    return s


def esmm_joint_backward(logits, d_logits, d_probs, d_cond, stream):
    """rk_esmm_joint_backward over contiguous [B, K] tensors (each incoming gradient may be None, not all):
    the gradient at the conditional logits, [B, K]."""
    B, K = logits.shape
    g = torch.empty(B, K, device=logits.device, dtype=torch.float32)
    check(_lib.load().rk_esmm_joint_backward(logits.data_ptr(), logits.stride(0), ptr(d_logits), ptr(d_probs),
                                             ptr(d_cond), K, B, K, g.data_ptr(), K, stream), "rk_esmm_joint_backward")
    return g


def esmm_backward(sh: EsmmShape, B, s, wst, towers, p, d_logits, d_probs, d_cond, need_dx, device):
    """The ESMM backward from the buffers of esmm_forward_train (s), the stacked layer-0 weight (wst) and
    the plain weights (towers: K (hidden [(W, b)…], (w, b))).  d_logits, d_probs, d_cond [B, K]: the incoming
    gradients, each may be None (not all).  Returns (dx [B, width] or None, tower grads [([(dW, db)…],
    (dw, db))…]); a db is returned for every layer.  The launches do not depend on K:
    rk_esmm_joint_backward; the heads and the layers above the first as mtl_tower_backward runs them for
    MMoE and PLE; layer 0 of all towers as one rk_gemm_wgrad against x and one rk_gemm against the stacked
    weight.  No float atomics, fixed-order sums."""
    K, width = sh.K, sh.width
    n0, p0, w4 = sh.tu[0], p4(sh.tu[0]), p4(width)
    st = _lib.raw_stream(device)
    g = esmm_joint_backward(s["logits"], d_logits, d_probs, d_cond, st)
    dz0, tower_grads = mtl_tower_backward(K, width, sh.tu, B, s["tacts"], None, None, towers, 1.0 / (1.0 - p), None, g,
                                          None, device, st, first=1)
    dWs, dbs = _wgrad(B, K * p0, w4, dz0, K * p0, s["x"], w4, device, st)
    dW0 = dWs.view(K, p0, w4)[:, :n0, :width].contiguous()   # one cut for all towers
    db0 = dbs.view(K, p0)[:, :n0].contiguous()
    for k in range(K):
        tower_grads[k][0][0] = (dW0[k], db0[k])
    dx = None
    if need_dx:
        dx = torch.empty(B, width, device=device, dtype=torch.float32)
        gemm(False, True, B, width, K * p0, dz0, K * p0, wst, wst.stride(0), dx, split=1)
    return dx, tower_grads


def esmm_flat_grads(sh: EsmmShape, tower_grads):
    """tower grads in the order tower-major: every hidden (dW, db), then the head's (dw, db)."""
    out = []
    for hidden, head in tower_grads:
        for wb in hidden:
            out += list(wb)
        out += list(head)
    return out


class _EsmmFn(torch.autograd.Function):
    """rankops.esmm with autograd: rk_esmm_forward_train without dropout, esmm_backward.  Inputs after the
    fixed arguments: x, then per tower every hidden (W, b) and the output (w, b) (None for an absent bias)."""

    @staticmethod
    def forward(ctx, sh, launch, x, *flat):
        s = launch()
        ctx.sh, ctx.s, ctx.flat, ctx.B = sh, s, flat, x.shape[0]
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None, not as zeros
        return s["probs"], s["logits"], s["cond"]

    @staticmethod
    def backward(ctx, d_probs, d_logits, d_cond):
        sh, s, flat, B = ctx.sh, ctx.s, ctx.flat, ctx.B
        towers, wst = s["weights"]
        dev = s["x"].device
        if B == 0 or (d_probs is None and d_logits is None and d_cond is None):
            return (None, None, torch.zeros(B, sh.width, device=dev)) + tuple(
                None if t is None else torch.zeros_like(t) for t in flat)
        like = lambda g: None if g is None else g.to(torch.float32).reshape(B, sh.K).contiguous()
        dx, tg = esmm_backward(sh, B, s, wst, towers, 0.0, like(d_logits), like(d_probs), like(d_cond),
                               ctx.needs_input_grad[2], dev)
        out = esmm_flat_grads(sh, tg)
        return (None, None, dx, *[None if t is None else g.reshape(t.shape) for t, g in zip(flat, out)])


def esmm(x: torch.Tensor, towers, return_conditional: bool = False):
    """The entire-space multi-task forward on rows x [B, width] (float32, unit column stride, any row
    stride >= width), in one launch (rk_esmm_forward):

        logit_k = towers[k](x)          towers: K (hidden [(W, b)…], (w_out [1, ·], b_out)), hidden layers
                                        Linear + ReLU, 1..3 of them; a bias may be None
        cond_k  = sigmoid(logit_k)      prob_k = cond_0 … cond_k  (k ascending)

    Returns (probs [B, K], logits [B, K]), with return_conditional also cond [B, K].  Differentiable
    whenever x or any weight or bias requires grad (rk_esmm_forward_train without dropout and
    esmm_backward): gradients for x and every (W, b) from the incoming gradients of
    probs, logits and cond.  With nothing requiring grad the call is the eval launch, bit for bit."""
    as_f32(x, "x")
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError(f"rankops.esmm: x must be [B, width] with unit column stride, got {tuple(x.shape)}")
    B, width = x.shape
    dev = x.device
    K = len(towers)
    if K == 0:
        raise ValueError("rankops.esmm: at least two towers")
    tstacks, heads, zero = [], [], None
    for k, (hidden, (w_out, b_out)) in enumerate(towers):
        st, last = _mmoe_stack(hidden, width, f"tower {k}", B > 0)
        as_f32(w_out, f"tower {k} output weight")
        if w_out.numel() != last or (b_out is not None and as_f32(b_out, f"tower {k} output bias").numel() != 1):
            raise ValueError(f"rankops.esmm: tower {k} output must be (w [1, {last}], b [1] or None)")
        if b_out is None:
            zero = torch.zeros(1, device=dev, dtype=torch.float32) if zero is None else zero
        tstacks.append(st)
        heads.append((w_out.detach().reshape(-1).contiguous(), zero if b_out is None else b_out.detach().reshape(1)))
    flat = [t for hidden, out in towers for wb in list(hidden) + [out] for t in wb]
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [x] + flat):
        tu = [w.shape[0] for w, _ in towers[0][0]]
        if len(tu) == 0 or any([w.shape[0] for w, _ in hidden] != tu for hidden, _ in towers):
            raise ValueError("rankops.esmm: with autograd all towers must have the same, non-empty widths")
        sh = EsmmShape(width, K, tu)
        dtow = [([(w.detach(), b) for w, b in hidden], (wo.detach().reshape(-1), bo)) for hidden, (wo, bo) in towers]
        wst = esmm_stacked_weight(sh, dtow) if B > 0 else None  # (an empty batch launches nothing)
        segs = [dense_segment(x.detach(), min(128, width - c), c, c) for c in range(0, width, 128)]

        def launch():
            s = esmm_forward_train(segs, sh, B, tstacks, heads, dev, 0.0, 0, None)
            s["weights"] = (dtow, wst)
            return s
        probs, logits, cond = _EsmmFn.apply(sh, launch, x, *flat)
        return (probs, logits, cond) if return_conditional else (probs, logits)
    f32 = dict(device=dev, dtype=torch.float32)
    probs, logits = torch.empty(B, K, **f32), torch.empty(B, K, **f32)
    cond = torch.empty(B, K, **f32) if return_conditional else None
    if B > 0:
        # (a segment holds at most 255 columns: the kernel's column map is one byte per column)
        segs = [dense_segment(x, min(128, width - c), c, c) for c in range(0, width, 128)]
        args, _keep = esmm_forward_args(segs, width, B, tstacks, heads, dev, logits=logits, probs=probs, cond=cond)
        args[-1] = _lib.raw_stream(dev)
        check(_lib.load().rk_esmm_forward(*args), "rk_esmm_forward")
    return (probs, logits, cond) if return_conditional else (probs, logits)


def esmm_loss_launch(logits, labels, weights, loss, per_task, dlogits):
    """rk_esmm_loss over logits / labels [B, K] (unit column stride, any row stride); weights: K floats or
    None; loss [1], per_task [K], dlogits [B, K] or None."""
    B, K = logits.shape
    lib = _lib.load()
    dev = logits.device
    _lib.ensure_device(dev)
    nws = lib.rk_esmm_loss_workspace_floats(B)
    ws = torch.empty(nws, device=dev, dtype=torch.float32)
    w = (ctypes.c_float * K)(*[float(v) for v in weights]) if weights is not None else None
    check(lib.rk_esmm_loss(logits.data_ptr(), logits.stride(0) if B else K, labels.data_ptr(),
                           labels.stride(0) if B else K, B, K, w, ptr(loss), ptr(per_task), ptr(dlogits),
                           dlogits.stride(0) if dlogits is not None and B else K, ws.data_ptr(), nws,
                           _lib.raw_stream(dev)), "rk_esmm_loss")


class _EsmmLossFn(torch.autograd.Function):
    """rankops.esmm_loss: the forward launches rk_esmm_loss with the analytic gradient, the backward is
    grad_out * dlogits.  The per-task means are returned detached."""

    @staticmethod
    def forward(ctx, logits, labels, weights):
        B, K = logits.shape
        f32 = dict(device=logits.device, dtype=torch.float32)
        loss, per_task = torch.empty((), **f32), torch.empty(K, **f32)
        dlogits = torch.empty(B, K, **f32) if ctx.needs_input_grad[0] else None
        esmm_loss_launch(logits, labels, weights, loss, per_task, dlogits)
        ctx.dlogits = dlogits
        ctx.mark_non_differentiable(per_task)
        return loss, per_task

    @staticmethod
    def backward(ctx, grad_loss, _grad_per_task):
        if ctx.dlogits is None or grad_loss is None:
            return None, None, None
        return grad_loss.to(torch.float32) * ctx.dlogits, None, None


def esmm_loss(logits: torch.Tensor, labels: torch.Tensor, task_weights=None, return_per_task: bool = False):
    """ESMM's entire-space loss, fused with its analytic gradient (rk_esmm_loss):

        (1 / B) sum_b [ w_0 BCE(sigmoid(z_0), y_0) + sum_{k >= 1} w_k BCE(sigmoid(z_0) … sigmoid(z_k), y_k) ]

    over conditional logits z [B, K] (any model's, when its tasks are nested events) and the joint events'
    labels y [B, K] in [0, 1], computed in the log domain so that saturated logits lose nothing.
    task_weights: K floats (default ones).  Returns the scalar loss, with return_per_task also the K
    unweighted per-task means (detached).  Differentiable in logits; capturable in a hipGraph."""
    as_f32(logits, "logits")
    require_gpu(labels, "labels")
    if logits.dim() != 2 or labels.shape != logits.shape:
        raise ValueError(f"rankops.esmm_loss: logits and labels must both be [B, K], got {tuple(logits.shape)} and "
                         f"{tuple(labels.shape)}")
    K = logits.shape[1]
    if not 1 <= K <= 8:
        raise ValueError(f"rankops.esmm_loss: 1..8 tasks, got {K}")
    if task_weights is not None:
        task_weights = tuple(float(v) for v in task_weights)
        if len(task_weights) != K:
            raise ValueError(f"rankops.esmm_loss: task_weights must hold {K} values, got {len(task_weights)}")
    labels = labels.detach().to(torch.float32)
    if logits.shape[0] and logits.stride(1) != 1:
        logits = logits.contiguous()
    if labels.shape[0] and labels.stride(1) != 1:
        labels = labels.contiguous()
    loss, per_task = _EsmmLossFn.apply(logits, labels, task_weights)
    return (loss, per_task) if return_per_task else loss
