"""Op-level GPU tests of the train-mode tail, DIN attention and AFM attention kernels
(csrc/train_bn.hip, train_din.hip, train_afm.hip): each rankops.ops wrapper is called directly with
preallocated tensors, the way rankops/train.py calls it, and compared with tests/train_ops_ref.py in
float64 on the CPU (forward outputs, and torch.autograd's gradients of a seeded scalar loss).

Comparison (close): per tensor max|got - want| <= REL[family] * max|want|, rtol 0, exact 0 where the
oracle's tensor is all zero, shape and float32 asserted.  Gathers, concatenations and "exact zero"
properties are compared with torch.equal / == 0.  Every output lives in a larger buffer pre-filled
with 777.0 whose other elements must come back bit-unchanged (a dead wave or a tail lane that
stores); accumulated outputs start from random values.

REL is not tuned on the kernels: it is 50 x the drift of the same restatement run in float32 on the
CPU against float64 over this file's case table (tests/test_train_ops_ref.py measures it and fails
if a constant here is below 50 x, or above 500 x, its family's drift); 50 is the margin
test_gpu_dien.py uses for hardware exp / rcp and another summation order.  Measured drifts
(max|f32 - f64| / max|f64|, worst tensor of the family) and the constants:

    family     fp32 drift   REL      worst tensor
    bn_act     1.17e-06     6e-5     dbeta at 63x1 (a sum of 63 signed terms)
    dice       7.06e-06     4e-4     dz at B = 1 (invstd = 316 multiplies two terms that cancel)
    prelu      1.50e-06     8e-5     the one-weight dweight at 65x130 (a sum of 4225 signed terms)
    din_pool   2.17e-07     1.2e-5   da2 at (7, 9, 48, 12), softmax
    din_fold   1.17e-07     7e-6     dq at (7, 9, 48)
    l2         9.78e-08     6e-6     the l2 term at 3 rows, 1 column
    afm_pool   8.83e-07     5e-5     dbd at (9, 6, 64, 256, 3)
    afm_fold   7.93e-08     5e-6     d_emb at (5, 16, 4, 65, 64)
    fm         2.32e-06     1.2e-4   dfinal_b at B = 255 (a sum of 255 signed terms)

The BN and Dice kernels reduce their statistics in fp64 and sit far inside these.  One tensor has no
usable max|want|: AFM's db2 = sum_{b,p} ds_{b,p} is 0 in exact arithmetic (the rows of a softmax's
Jacobian sum to zero), so the oracle's value is its own rounding noise; db2 is compared on the scale
of its summands, sum|ds| from the oracle (train_ops_ref.afm_pool_eval), with the family's REL.

With BatchNorm on, the sign of a pre-activation within rounding of zero could differ between fp32
and fp64; the case table's seeds keep every |u| >= 1e-5 max|u| (asserted on the CPU), so no element
is left out of any comparison."""
from types import SimpleNamespace as NS

import pytest
import torch

import rankops
import train_ops_ref as R
from rankops import _lib, ops

pytestmark = pytest.mark.gpu

REL = {"bn_act": 6e-5, "dice": 4e-4, "prelu": 8e-5, "din_pool": 1.2e-5, "din_fold": 7e-6, "l2": 6e-6,
       "afm_pool": 5e-5, "afm_fold": 5e-6, "fm": 1.2e-4}
SENT = 777.0
RK_ERR_INVALID = 1  # include/rankops.h
f64 = torch.float64


def close(name, got, want, rel, scale=None):
    assert got.dtype == torch.float32 and want.dtype == f64, name
    got = got.detach().double().cpu()
    assert got.shape == want.shape, f"{name}: {tuple(got.shape)} != {tuple(want.shape)}"
    _, err, scale = R.rel_err(got, want, scale)
    print(f"{name}: max |err| = {err:.3e}, max |want| = {scale:.3e}")
    if scale == 0.0:
        assert err == 0.0, f"{name}: the oracle's tensor is all zero, got {err:.3e}"
    else:
        assert err <= rel * scale, f"{name}: {err:.3e} > {rel} * {scale:.3e}"


class Guard:
    """A (rows, cols) window at column c0 of a sentinel-filled (rows + 2, c0 + cols + pad) buffer."""

    def __init__(self, rows, cols, c0=0, pad=0, fill=None):
        self.buf = torch.full((rows + 2, c0 + cols + pad), SENT, device="cuda")
        self.box = (rows, c0, cols)
        self.v = self.buf[:rows, c0:c0 + cols]
        if fill is not None:
            self.v.copy_(fill)

    def check(self, what=""):
        rows, c0, cols = self.box
        rest = self.buf.clone()
        rest[:rows, c0:c0 + cols] = SENT
        assert bool((rest == SENT).all()), f"{what}: stored outside its range"
        return self.v


class Flat:
    """A contiguous tensor of `shape` at element `offset` of a sentinel-filled flat buffer."""

    def __init__(self, *shape, offset=0, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((offset + n + 67,), SENT, device="cuda")
        self.span = (offset, n)
        self.v = self.buf[offset:offset + n].view(*shape)
        if fill is not None:
            self.v.copy_(fill)

    def check(self, what=""):
        o, n = self.span
        assert bool((self.buf[:o] == SENT).all()) and bool((self.buf[o + n:] == SENT).all()), \
            f"{what}: stored outside its range"
        return self.v


def cuda(t):
    return None if t is None else t.cuda()


def all_zero(t):
    return bool((t == 0).all())


def rng_slot(start=5):
    counter = torch.full((1,), start, dtype=torch.int64, device="cuda")
    slot = torch.empty(1, dtype=torch.int64, device="cuda")
    ops.rng_next(counter, slot)
    assert int(slot) == start and int(counter) == start + 1
    return counter, slot


def window(B, N, strided, fill=None):
    return Guard(B, N, c0=1, pad=2, fill=fill) if strided else Guard(B, N, fill=fill)


def invalid(fn, *a, **kw):
    with pytest.raises(_lib.RankOpsError) as e:
        fn(*a, **kw)
    assert e.value.code == RK_ERR_INVALID


# ------------------------------------------------------------------ BN + activation + dropout

def make_bn(i, N, affine=True):
    bn = torch.nn.BatchNorm1d(N, eps=R.BN_EPS, momentum=R.BN_MOMENTUM, affine=affine).cuda().train()
    with torch.no_grad():
        if affine:
            bn.weight.copy_(i.gamma)
            bn.bias.copy_(i.beta)
        bn.running_mean.copy_(i.running_mean)
        bn.running_var.copy_(i.running_var)
    return bn


@pytest.mark.parametrize("case", R.BN_CASES, ids=R.bn_id)
def test_bn_act_forward_backward(case):
    B, N, bn_on, act, slope, p, has_bias = case
    i = R.bn_inputs(case)
    strided = has_bias  # z, y, dy, dz as column slices of wider buffers
    bn = make_bn(i, N) if bn_on else None
    bias, seed = cuda(i.bias), 1234 + B
    counter, slot = rng_slot()
    mask = ops.dropout_mask(seed, slot, B, N, p) if p > 0 else None
    z, y, dy, dz = (window(B, N, strided, fill=f) for f in (i.z, None, i.G, None))
    mean, invstd, dgamma, dbeta = (Flat(N) for _ in range(4))
    ws = torch.empty(2 * N, device="cuda", dtype=f64)
    ops.bn_act_train_forward(z.v, bias, bn, act, p, seed, slot, y.v, mean.v, invstd.v, ws, slope=slope)
    ops.bn_act_backward(dy.v, z.v, bias, bn, act, p, seed, slot, mean.v, invstd.v, ws, dz.v,
                        dgamma.v if bn_on else None, dbeta.v if bn_on else None, slope=slope)
    torch.cuda.synchronize()
    want = R.bn_eval(case, i, f64, None if mask is None else mask.cpu())
    rel = REL["bn_act"]
    close("y", y.check("y"), want["y"], rel)
    close("dz", dz.check("dz"), want["dz"], rel)
    for g in (z, dy):
        g.check("input")
    if mask is not None:  # dropped elements are exact zeros
        assert all_zero(y.v[mask == 0])
        if not bn_on:  # (with BN a dropped element still gets gradient through the batch statistics)
            assert all_zero(dz.v[mask == 0])
    if bn_on:
        close("save_mean", mean.check("save_mean"), want["save_mean"], rel)
        close("save_invstd", invstd.check("save_invstd"), want["save_invstd"], rel)
        close("running_mean", bn.running_mean, want["running_mean"], rel)
        close("running_var", bn.running_var, want["running_var"], rel)
        assert int(bn.num_batches_tracked) == 1
        close("dgamma", dgamma.check("dgamma"), want["dgamma"], rel)
        close("dbeta", dbeta.check("dbeta"), want["dbeta"], rel)
    else:
        for f in (mean, invstd, dgamma, dbeta):
            f.check("unused statistics")
            assert bool((f.v == SENT).all())
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("B,N", R.BN_SHAPES)
def test_bn_without_affine_or_running_statistics(B, N):
    """gamma / beta / running statistics are optional (BatchNorm1d(affine=False,
    track_running_stats=False)): no dgamma / dbeta is asked for."""
    case = (B, N, True, "relu", 0.0, 0.0, True)
    i = R.bn_inputs(case)
    bn = torch.nn.BatchNorm1d(N, eps=R.BN_EPS, affine=False, track_running_stats=False).cuda().train()
    z, y, dy, dz = (window(B, N, True, fill=f) for f in (i.z, None, i.G, None))
    mean, invstd = Flat(N), Flat(N)
    ws = torch.empty(2 * N, device="cuda", dtype=f64)
    ops.bn_act_train_forward(z.v, cuda(i.bias), bn, True, 0.0, 0, None, y.v, mean.v, invstd.v, ws)
    ops.bn_act_backward(dy.v, z.v, cuda(i.bias), bn, True, 0.0, 0, None, mean.v, invstd.v, ws, dz.v, None, None)
    zl = i.z.double().requires_grad_(True)
    u = R.bn_pre(zl.detach(), i.bias.double(), None, None, R.BN_EPS)[0]
    keep = ~R.near_zero(u)  # the seeds were chosen for the affine u: leave out what sits on zero here
    assert float(keep.double().mean()) >= 0.999
    yw = R.bn_act(zl, i.bias.double(), None, None, R.BN_EPS, "relu", 0.0, None)[0]
    dzw = torch.autograd.grad((yw * i.G.double()).sum(), zl)[0]
    close("y", y.check("y") * keep.cuda(), yw.detach() * keep, REL["bn_act"])
    close("dz", dz.check("dz") * keep.cuda(), dzw * keep, REL["bn_act"])
    assert rankops.error_flags() == 0


def test_dropout_mask_is_one_hash_for_forward_backward_and_mask():
    """Without BN and activation, dy = 1 gives dz = the mask and z = 1 gives y = the mask, bit for
    bit: forward, backward and rk_dropout_mask hash the same element index; rk_rng_next moves on."""
    B, N, p, seed = 65, 130, 0.25, 99
    counter, slot = rng_slot(7)
    mask = ops.dropout_mask(seed, slot, B, N, p)
    scale = float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))
    assert bool(((mask == 0) | (mask == scale)).all())
    assert abs(float((mask == 0).float().mean()) - p) < 0.02  # 8450 draws: four standard deviations
    ones, y, dz = window(B, N, True, fill=torch.ones(B, N)), window(B, N, True), window(B, N, False)
    ops.bn_act_train_forward(ones.v, None, None, False, p, seed, slot, y.v, None, None, None)
    ops.bn_act_backward(ones.v, ones.v, None, None, False, p, seed, slot, None, None, None, dz.v, None, None)
    assert torch.equal(y.check("y"), mask) and torch.equal(dz.check("dz"), mask)
    assert not torch.equal(ops.dropout_mask(seed + 1, slot, B, N, p), mask)  # another unit's seed
    slot2 = torch.empty_like(slot)
    ops.rng_next(counter, slot2)
    assert int(slot2) == 8 and int(counter) == 9
    mask2 = ops.dropout_mask(seed, slot2, B, N, p)
    assert not torch.equal(mask2, mask)
    ops.bn_act_backward(ones.v, ones.v, None, None, False, p, seed, slot2, None, None, None, dz.v, None, None)
    assert torch.equal(dz.check("dz"), mask2)
    assert rankops.error_flags() == 0


def test_bn_and_dice_backward_refuse_short_leading_dimensions():
    """A row stride below the width would alias rows: RK_ERR_INVALID, as the forwards answer."""
    B, N = 5, 8
    full = torch.zeros(B, N, device="cuda")
    short = torch.zeros(B * N, device="cuda").as_strided((B, N), (N - 1, 1))
    mean, invstd = torch.zeros(N, device="cuda"), torch.ones(N, device="cuda")
    ws = torch.empty(3 * N, device="cuda", dtype=f64)
    dice = NS(alpha=torch.zeros(N, device="cuda"), bn=torch.nn.BatchNorm1d(N, affine=False).cuda())
    prelu = torch.nn.PReLU().cuda()
    for k in range(3):
        a = [short if j == k else full for j in range(3)]  # dy, z, dz
        invalid(ops.bn_act_backward, a[0], a[1], None, None, True, 0.0, 0, None, None, None, None, a[2], None, None)
        invalid(ops.dice_backward, a[0], a[1], None, dice, mean, invstd, ws, a[2], None)
        invalid(ops.prelu_backward, a[0], a[1], None, prelu, ws, a[2], None)
    invalid(ops.bn_act_train_forward, short, None, None, True, 0.0, 0, None, full, None, None, None)
    invalid(ops.dice_train_forward, full, None, dice, short, mean, invstd, ws)
    invalid(ops.prelu_train_forward, short, None, prelu, full)
    assert int(dice.bn.num_batches_tracked) == 0
    assert rankops.error_flags() == 0


# ------------------------------------------------------------------ Dice and PReLU

@pytest.mark.parametrize("case", R.DICE_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{'bias' if c[2] else 'nobias'}")
def test_dice_forward_backward(case):
    B, N, has_bias = case
    i = R.dice_inputs(case)
    dice = NS(alpha=i.alpha.cuda(), bn=make_bn(i, N, affine=False))
    z, y, dy, dz = (window(B, N, has_bias, fill=f) for f in (i.z, None, i.G, None))
    mean, invstd, dalpha = Flat(N), Flat(N), Flat(N)
    ops.dice_train_forward(z.v, cuda(i.bias), dice, y.v, mean.v, invstd.v, torch.empty(2 * N, device="cuda", dtype=f64))
    ops.dice_backward(dy.v, z.v, cuda(i.bias), dice, mean.v, invstd.v, torch.empty(3 * N, device="cuda", dtype=f64),
                      dz.v, dalpha.v)
    want, rel = R.dice_eval(case, i, f64), REL["dice"]
    close("y", y.check("y"), want["y"], rel)
    close("save_mean", mean.check("save_mean"), want["save_mean"], rel)
    close("save_invstd", invstd.check("save_invstd"), want["save_invstd"], rel)
    close("running_mean", dice.bn.running_mean, want["running_mean"], rel)
    close("running_var", dice.bn.running_var, want["running_var"], rel)
    assert int(dice.bn.num_batches_tracked) == 1
    close("dz", dz.check("dz"), want["dz"], rel)
    close("dalpha", dalpha.check("dalpha"), want["dalpha"], rel)
    z.check("z")
    dy.check("dy")
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("case", R.PRELU_CASES,
                         ids=lambda c: f"{c[0]}x{c[1]}-{'percol' if c[2] else 'one'}-{'bias' if c[3] else 'nobias'}")
def test_prelu_forward_backward(case):
    B, N, per_col, has_bias = case
    i = R.prelu_inputs(case)
    prelu = torch.nn.PReLU(N if per_col else 1).cuda()
    with torch.no_grad():
        prelu.weight.copy_(i.weight)
    nw = prelu.weight.numel()
    z, y, dy, dz = (window(B, N, has_bias, fill=f) for f in (i.z, None, i.G, None))
    dweight = Flat(nw)
    ops.prelu_train_forward(z.v, cuda(i.bias), prelu, y.v)
    ops.prelu_backward(dy.v, z.v, cuda(i.bias), prelu, torch.empty(nw, device="cuda", dtype=f64), dz.v, dweight.v)
    want, rel = R.prelu_eval(case, i, f64), REL["prelu"]
    close("y", y.check("y"), want["y"], rel)
    close("dz", dz.check("dz"), want["dz"], rel)
    close("dweight", dweight.check("dweight"), want["dweight"], rel)
    x0 = (want["y"] == 0)  # the exact zeros of x: y = 0, dz = dy * weight
    assert int(x0.sum()) >= min(3, B * N) - 1 and all_zero(y.v.cpu()[x0])
    assert rankops.error_flags() == 0


# ------------------------------------------------------------------ DIN attention training

def run_din_pool(shape, i, softmax, offset=0):
    """rk_din_att_pool_forward / _backward on shape's inputs; a2 / da2 / keys / dkeys at `offset` floats."""
    B, T, H, A2 = shape
    att_col, width = 5, 5 + H + 3
    a2 = Flat(B * T, A2, offset=offset, fill=i.a2)
    keys = Flat(B, T, H, offset=offset, fill=i.keys)
    w3, b3, lens = i.w3.cuda(), i.b3.cuda(), i.lens.cuda()
    wts, x = Flat(B, T), Guard(B, H, c0=att_col, pad=3)
    ops.din_att_pool_forward(a2.v, w3, b3, keys.v, lens, T, H, softmax, wts.v, x.buf[:B], att_col)
    dx = torch.randn(B, width, device="cuda")
    dx[:, att_col:att_col + H] = i.dout.cuda()
    dx0 = dx.clone()
    dkeys, da2 = Flat(B, T, H, offset=offset), Flat(B * T, A2, offset=offset)
    ops.din_att_pool_backward(dx, att_col, wts.v, keys.v, a2.v, w3, lens, T, H, softmax, dkeys.v, da2.v)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx0)
    for g in (a2, keys):
        g.check("input")
    return dict(weights=wts.check("weights"), out=x.check("attention columns"), dkeys=dkeys.check("dkeys"),
                da2=da2.check("da2"))


@pytest.mark.parametrize("softmax", [False, True], ids=["masked", "softmax"])
@pytest.mark.parametrize("shape", R.DIN_SHAPES, ids=str)
def test_din_att_pool_forward_backward(shape, softmax):
    B, T, H, A2 = shape
    i = R.din_inputs(shape)
    got, want = run_din_pool(shape, i, softmax), R.din_pool_eval(shape, i, f64, softmax)
    for n in ("weights", "out", "dkeys", "da2"):
        close(n, got[n], want[n], REL["din_pool"])
    past = (torch.arange(T)[None, :] >= i.lens[:, None])
    free = past & ~(i.lens == 0)[:, None] if softmax else past  # softmax over no key: weights 1 / T
    dkeys, da2 = got["dkeys"].cpu(), got["da2"].cpu().view(B, T, A2)
    assert all_zero(dkeys[free]) and all_zero(da2[past]) and all_zero(da2[i.a2.view(B, T, A2) == 0])
    if softmax and bool((i.lens == 0).any()):
        e = i.lens == 0
        assert torch.equal(got["weights"].cpu()[e], torch.full((int(e.sum()), T), 1.0, dtype=torch.float32) / T)
        close("dkeys of the empty sample", got["dkeys"][e.cuda()], (i.dout[e].double() / T)[:, None, :].expand(-1, T, H),
              REL["din_pool"])
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("softmax", [False, True], ids=["masked", "softmax"])
def test_din_att_pool_at_a_one_float_offset_takes_the_scalar_path(softmax):
    shape = (6, 65, 16, 40)  # float4-eligible: H % 4 == 0, A2 % 4 == 0
    i = R.din_inputs(shape)
    want = R.din_pool_eval(shape, i, f64, softmax)
    aligned, shifted = run_din_pool(shape, i, softmax), run_din_pool(shape, i, softmax, offset=1)
    assert aligned["dkeys"].data_ptr() % 16 == 0 and shifted["dkeys"].data_ptr() % 16 == 4
    for n in ("weights", "out", "dkeys", "da2"):
        close(n + " (offset)", shifted[n], want[n], REL["din_pool"])
        close(n + " (offset against aligned)", shifted[n], aligned[n].double().cpu(), REL["din_pool"])
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("shape", [s[:3] for s in R.DIN_SHAPES], ids=str)
def test_din_att_cross_is_the_gather_and_concatenation(shape):
    B, T, H = shape
    i = R.din_inputs(next(s for s in R.DIN_SHAPES if s[:3] == shape))
    q_col, width = 3, 3 + H + 2  # the query is not 16-B aligned
    x = torch.full((B, width), SENT, device="cuda")
    x[:, q_col:q_col + H] = i.q.cuda()
    table = i.table.cuda()
    for ids in (i.ids, None):
        if ids is None:  # out-of-range ids: zero key rows and the flag; the neighbours stay right
            ids = i.ids.clone()
            ids[0, 0] = -1
            ids[-1, -1] = R.DIN_VOCAB + 3
            bad = (ids < 0) | (ids >= R.DIN_VOCAB)
        else:
            bad = torch.zeros_like(ids, dtype=torch.bool)
        keys, cross = Flat(B, T, H), Flat(B * T, 4 * H)
        ops.din_att_cross(x, q_col, table, ids.cuda(), T, H, keys.v, cross.v)
        want_keys = i.table[ids.clamp(0, R.DIN_VOCAB - 1)] * (~bad)[:, :, None]
        qe = i.q[:, None, :].expand(B, T, H)
        want_cross = torch.cat([qe, want_keys, qe - want_keys, qe * want_keys], 2).reshape(B * T, 4 * H)
        assert torch.equal(keys.check("keys").cpu(), want_keys)
        assert torch.equal(cross.check("cross").cpu(), want_cross)
        assert torch.equal(cross.v.cpu(), R.din_cross(i.q, want_keys).reshape(B * T, 4 * H))
        assert rankops.error_flags() == (_lib.RK_FLAG_INDEX_OOB if bad.any() else 0)
    assert rankops.error_flags() == 0  # reading the flags reset them


@pytest.mark.parametrize("shape", R.FOLD_SHAPES, ids=str)
def test_din_cross_fold_accumulates_into_dkeys_and_the_query_columns(shape):
    B, T, H = shape
    i = R.fold_inputs(shape)
    q_col, width = 3, 3 + H + 2
    x = torch.full((B, width), SENT, device="cuda")
    x[:, q_col:q_col + H] = i.q.cuda()
    dx = torch.randn(B, width, device="cuda")
    dx[:, q_col:q_col + H] = i.dq0.cuda()
    dx0 = dx.clone()
    dkeys = Flat(B, T, H, fill=i.dkeys0)
    ops.din_cross_fold(i.dcross.cuda(), x, q_col, i.keys.cuda(), T, H, dkeys.v, dx)
    want = R.fold_eval(shape, i, f64)
    close("dkeys", dkeys.check("dkeys"), want["dkeys"], REL["din_fold"])
    close("dq", dx[:, q_col:q_col + H], want["dq"], REL["din_fold"])
    keep = [c for c in range(width) if not q_col <= c < q_col + H]
    assert torch.equal(dx[:, keep], dx0[:, keep])
    assert rankops.error_flags() == 0


def test_din_att_pool_refuses_shapes_past_its_limits():
    for B, T, H in ((2, 3, 65), (1, 1025, 8)):
        A2 = 4
        a2, keys = torch.zeros(B * T, A2, device="cuda"), torch.zeros(B, T, H, device="cuda")
        w3, b3 = torch.zeros(A2, device="cuda"), torch.zeros(1, device="cuda")
        lens = torch.ones(B, dtype=torch.int64, device="cuda")
        wts, x = Flat(B, T), Guard(B, H)
        invalid(ops.din_att_pool_forward, a2, w3, b3, keys, lens, T, H, False, wts.v, x.v, 0)
        dkeys, da2 = Flat(B, T, H), Flat(B * T, A2)
        invalid(ops.din_att_pool_backward, x.v, 0, wts.v, keys, a2, w3, lens, T, H, True, dkeys.v, da2.v)
        for g in (wts, x, dkeys, da2):
            g.check("refused call")
            assert bool((g.v == SENT).all())
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("case", R.L2_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_row_l2norm_mean_and_backward(case):
    rows, ncols = case
    i = R.l2_inputs(case)
    c0 = R.L2_COL0
    x, out = i.x.cuda(), Flat(1)
    ops.row_l2norm_mean(x, c0, ncols, R.L2_LAMBDA, out.v.view(()))
    dx = i.dx0.cuda()
    gout = torch.tensor([R.L2_GOUT], device="cuda")  # read from device memory
    ops.row_l2norm_backward(x, c0, ncols, R.L2_LAMBDA / rows, gout, dx)
    want = R.l2_eval(case, i, f64)
    close("l2", out.check("l2"), want["l2"], REL["l2"])
    close("dx", dx[:, c0:c0 + ncols], want["dx"], REL["l2"])
    keep = [c for c in range(dx.shape[1]) if not c0 <= c < c0 + ncols]
    assert torch.equal(dx[:, keep].cpu(), i.dx0[:, keep])
    assert bool(torch.isfinite(dx).all())
    if rows > 1:  # the zero-norm row: torch.norm's zero subgradient, dx untouched
        assert torch.equal(dx[1].cpu(), i.dx0[1])
    assert rankops.error_flags() == 0


# ------------------------------------------------------------------ AFM training

def afm_dims(shape):
    B, Fn, D, A, nd = shape
    return B, Fn, D, A, nd, Fn * (Fn - 1) // 2


@pytest.mark.parametrize("shape", R.AFM_SHAPES, ids=str)
def test_afm_pairs_is_the_gather_and_products(shape):
    B, Fn, D, A, nd, P = afm_dims(shape)
    i = R.afm_inputs(shape)
    tables = [t.cuda() for t in i.tables]
    for oob in (False, True):
        idx = [x.clone() for x in i.idx]
        if oob:
            idx[0][0] = -1
            idx[-1][-1] = R.AFM_VOCAB + 3
        didx = [x.cuda() for x in idx]
        emb, pairs = Flat(B, Fn * D), Flat(B * P, D)
        ops.afm_pairs([ops.table_segment(t, x, 0) for t, x in zip(tables, didx)], D, B, emb.v, pairs.v)
        want = torch.stack([t[x.clamp(0, R.AFM_VOCAB - 1)] * ((x >= 0) & (x < R.AFM_VOCAB))[:, None]
                            for t, x in zip(i.tables, idx)], 1)
        assert torch.equal(emb.check("emb").cpu(), want.reshape(B, Fn * D))
        assert torch.equal(pairs.check("pairs").cpu(), R.afm_pairs(want).reshape(B * P, D))
        assert rankops.error_flags() == (_lib.RK_FLAG_INDEX_OOB if oob else 0)


def run_afm_pool_forward(shape, i):
    B, Fn, D, A, nd, P = afm_dims(shape)
    d = NS(a1=i.a1.cuda(), pairs=i.pairs.reshape(B * P, D).cuda(), dense=Guard(B, nd, c0=1, pad=1, fill=i.dense))
    for n in ("w2", "b2", "wd", "bd", "wp", "bp"):
        setattr(d, n, getattr(i, n).cuda())
    d.weights, d.ws, d.logit, d.pred = Flat(B, P), Flat(B, D), Flat(B, 1), Flat(B, 1)
    ops.afm_pool_forward(d.a1, d.w2, d.b2, d.pairs, P, D, d.dense.v, d.wd, d.bd, d.wp, d.bp, d.weights.v, d.ws.v,
                         d.logit.v, d.pred.v)
    return d


@pytest.mark.parametrize("mode", R.AFM_MODES)
@pytest.mark.parametrize("shape", R.AFM_SHAPES, ids=str)
def test_afm_pool_forward_backward(shape, mode):
    B, Fn, D, A, nd, P = afm_dims(shape)
    i = R.afm_inputs(shape)
    want, rel = R.afm_pool_eval(shape, i, f64, mode), REL["afm_pool"]
    d = run_afm_pool_forward(shape, i)
    close("weights", d.weights.check("weights"), want["weights"], rel)
    close("ws", d.ws.check("ws"), want["ws"], rel)
    close("logit", d.logit.check("logit").view(B), want["logit"], rel)
    close("pred", d.pred.check("pred").view(B), want["pred"], rel)
    d_pairs, da1, acc = Flat(B * P, D), Flat(B * P, A), Flat(nd + 1 + D + 1 + A + 1)
    ops.afm_pool_backward(i.dpred.cuda() if mode != "dtotal" else None, i.dtotal.cuda() if mode != "dpred" else None,
                          d.pred.v, d.weights.v, d.ws.v, d.pairs, d.a1, d.w2, d.wp, d.dense.v, P, D, d_pairs.v, da1.v,
                          acc.v)
    close("d_pairs", d_pairs.check("d_pairs"), want["d_pairs"], rel)  # overwritten: it started as the sentinel
    close("da1", da1.check("da1"), want["da1"], rel)
    assert all_zero(da1.v.cpu()[i.a1 == 0])
    acc.check("acc")
    o = 0
    for n, k in (("dwd", nd), ("dbd", 1), ("dwp", D), ("dbp", 1), ("dw2", A), ("db2", 1)):
        close(n, acc.v[o:o + k], want[n], rel, want.get("scale:" + n))  # db2: on the scale of its summands
        o += k
    d.dense.check("dense")
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("shape", R.AFM_SHAPES, ids=str)
def test_afm_pair_fold(shape):
    B, Fn, D, A, nd, P = afm_dims(shape)
    i = R.afm_inputs(shape)
    d_emb = Flat(B, Fn * D)
    ops.afm_pair_fold(i.d_pairs.cuda(), i.emb.reshape(B, Fn * D).cuda(), Fn, D, d_emb.v)
    close("d_emb", d_emb.check("d_emb"), R.afm_fold_eval(shape, i, f64)["d_emb"], REL["afm_fold"])
    assert rankops.error_flags() == 0


def test_afm_refuses_shapes_past_its_limits():
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    B, D = 2, 4
    idx = torch.zeros(B, dtype=torch.int64, device="cuda")
    table = z(3, D)
    for Fn in (17, 1):
        P = max(1, Fn * (Fn - 1) // 2)
        emb, pairs, d_emb = Flat(B, Fn * D), Flat(B * P, D), Flat(B, Fn * D)
        invalid(ops.afm_pairs, [ops.table_segment(table, idx, 0)] * Fn, D, B, emb.v, pairs.v)
        invalid(ops.afm_pair_fold, z(B * P, D), z(B, Fn * D), Fn, D, d_emb.v)
        for g in (emb, pairs, d_emb):
            g.check("refused call")
            assert bool((g.v == SENT).all())

    def pool(P, D, A, nd, forward):
        a1, pairs, dense = z(B * P, A), z(B * P, D), z(B, nd)
        out = [Flat(B, P), Flat(B, D), Flat(B, 1), Flat(B, 1), Flat(B * P, D), Flat(B * P, A), Flat(nd + D + A + 3)]
        w, ws, logit, pred, d_pairs, da1, acc = (f.v for f in out)
        if forward:
            invalid(ops.afm_pool_forward, a1, z(A), z(1), pairs, P, D, dense, z(nd), z(1), z(D), z(1), w, ws, logit,
                    pred)
        invalid(ops.afm_pool_backward, z(B), None, z(B, 1), z(B, P), z(B, D), pairs, a1, z(A), z(D), dense, P, D,
                d_pairs, da1, acc)
        for f in out:
            f.check("refused call")
            assert bool((f.v == SENT).all())

    pool(3, D, 257, 2, forward=False)   # the backward stages dw2 in LDS: A <= 256 (the forward takes any A)
    pool(3, 65, 8, 2, forward=True)     # one lane per embedding column: D <= 64
    pool(136, D, 8, 2, forward=True)    # 17 fields' pairs
    pool(3, D, 8, 65, forward=True)     # one lane per dense column
    assert rankops.error_flags() == 0


# ------------------------------------------------------------------ DeepFM pieces

@pytest.mark.parametrize("mode", R.FM_MODES)
@pytest.mark.parametrize("shape", R.FM_SHAPES, ids=str)
def test_fm_backward(shape, mode):
    B, Fn, D = shape
    i = R.fm_inputs(shape)
    deep_in = Guard(B, Fn * D, c0=1, pad=2, fill=i.e.reshape(B, Fn * D))
    d_deep = Guard(B, Fn * D, c0=2, pad=0, fill=i.d_deep) if mode != "no_d_deep" else None
    dfm2 = i.dfm2.cuda().view(B, 1) if mode != "no_dfm2" else None
    out = Guard(B, Fn * D, c0=3, pad=1)
    ops.fm_backward(deep_in.v, None if d_deep is None else d_deep.v, dfm2, Fn, D, out.v)
    close("d_e", out.check("d_e"), R.fm_eval(shape, i, f64, mode)["d_e"], REL["fm"])
    deep_in.check("deep_in")
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("case", R.COMBINE_CASES, ids=lambda c: f"{c[0]}-no_{c[1]}")
def test_fm_combine_backward(case):
    B, none = case
    i = R.combine_inputs(case)
    want = R.combine_eval(case, i, f64)
    prob = want["prob"].float().cuda().view(B, 1)
    go = [None if n == none else getattr(i, n).cuda().view(B, 1) for n in R.COMBINE_GRADS]
    dfm1, dfm2, ddeep = Flat(B, 1), Flat(B, 1), Flat(B, 1)
    dw, db = Flat(1, 3), Flat(1)  # start from the sentinel: the host function zeroes them
    ops.fm_combine_backward(*go, prob, i.fm1.cuda().view(B, 1), i.fm2.cuda().view(B, 1), i.deep.cuda().view(B, 1),
                            i.w.cuda().view(1, 3), dfm1.v, dfm2.v, ddeep.v, dw.v, db.v)
    rel = REL["fm"]
    for n, g in (("dfm1", dfm1), ("dfm2", dfm2), ("ddeep", ddeep)):
        close(n, g.check(n).view(B), want[n], rel)
    close("dfinal_w", dw.check("dfinal_w").view(3), want["dfinal_w"], rel)
    close("dfinal_b", db.check("dfinal_b"), want["dfinal_b"], rel)
    assert rankops.error_flags() == 0
