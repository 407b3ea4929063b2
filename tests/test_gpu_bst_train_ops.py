"""Op-level GPU tests of the BST training kernels (csrc/train_bst.hip): each rankops.ops wrapper is
called directly with preallocated tensors, the way rankops/train.py calls it, and compared with
tests/bst_train_ref.py in float64 on the CPU (forward outputs, torch.autograd's gradients).  Dropout
masks are the engine's own (ops.dropout_mask: the same counter hash and element index m * d + k; the
flat element for leaky_dropout).

Comparison (test_gpu_train_ops.close): per tensor max|got - want| <= REL[family] * max|want|, rtol 0.
Every output lives in a larger buffer pre-filled with 777.0 whose other elements must come back
bit-unchanged; accumulated outputs (dpos) start from random values, overwritten ones (dqkv, dr,
dgamma, ...) from the sentinel, which proves them fully overwritten.

REL is not tuned on the kernels: it is 100 x the drift of the same restatement run in float32 on the
CPU against float64 over this file's case table, rounded to two digits (tests/test_bst_train_ref.py
measures it and fails if a constant here is below 50 x, or above 500 x, its family's drift; 50 is the
margin the project uses for hardware exp / rcp and another summation order, and the factor 2 above
it is room for a CPU whose BLAS sums in another order than the one these were measured on).  The
attention kernels use FP32 MFMA (v_mfma_f32_16x16x4_f32), full fp32: no wider allowance.  Measured
drifts (max|f32 - f64| / max|f64|, worst tensor of the family) and the constants:

    family       fp32 drift   REL      worst tensor
    att          5.19e-07     5e-5     P at (N4, 64, 64, 1)
    ln_fwd       2.34e-07     2.4e-5   y at (9, 50), p = 0
    ln_fwd_big   2.68e-06     2.7e-4   y at the grid-clamp case, p = 0.1 (the worst of 524365 rows of 4
                                       columns: a small variance amplifies the rounding of r - mean)
    ln_bwd       2.65e-07     2.7e-5   dgamma at (7, 6), p = 0
    ln_bwd_big   5.59e-07     5.6e-5   dgamma at the grid-clamp case (a sum of 524365 signed terms)
    pos          1.57e-07     1.6e-5   dpos at B = 130, (T, d) = (5, 6)
    pool         1.68e-07     1.7e-5   the pooled row at T = 70, d = 6, sum pooling
    leaky        8.84e-08     9e-6     df at n = 1, p = 0.1

One quantity is zero in exact arithmetic: dbk = sum over the rows of dK (the gradient of w_k's bias;
sum_j dS[i, j] = 0).  It is no output of the attention kernels, but it is what a wrong dK would
corrupt unseen, so it is compared on the scale of its summands (bst_train_ref.att_eval).
seq_len = 0 makes a row of -inf, NaN in the oracle as well: out of scope.  LeakyReLU's sign is taken
from the same fp32 f on both sides, so no element of any comparison is left out.

Which case reaches which path, from the dispatch at the bottom of train_bst.hip.  Attention
(B, T, d, heads), dh = d / heads, TP / DP = T / dh padded to 16, NS = TP / 16 strips; the persistent
kernels need dh % 4 == 0 and T % 4 == 0, US = 1 / 2 / 4 for TP * DP / 4 <= 256 / <= 512 / above:
    (3, 5, 6, 2)      one-item kernels, dh = 3: att_stage's scalar branch, scalar P
    (3, 8, 6, 2)      one-item kernels, dh = 3 with T % 4 == 0: scalar staging, float4 P
    (2, 18, 8, 2)     one-item kernels, dh = 4, T % 4 = 2: att_stage_all, scalar P, NS = 2
    (3, 17, 12, 1)    one-item kernels, T one past a 16 boundary, DP = 16 filled to 12
    (2, 1, 4, 1)      one-item kernels, T = 1
    (N1, 4, 16, 4)    persistent US = 1 (16 * 16 / 4 = 64 slots), looping
    (2, 20, 80, 2)    persistent US = 2, 32 * 48 / 4 = 384 of 512 slots: the `i < n` guard
    (N2, 32, 64, 1)   persistent US = 2 full (32 * 64 / 4 = 512), looping
    (2, 44, 104, 2)   persistent US = 4, 48 * 64 / 4 = 768 of 1024 slots, rows and columns padded
    (N4, 64, 64, 1)   persistent US = 4 full, the 104448-byte backward (raised LDS limit), looping
The looping batches N are bst_train_ref.loop_batch: B * heads >= 2 * bound + 3 with bound = num_cus *
min(8, 160 KiB / lds_bytes), per direction (the backward runs the first N_bwd samples of the forward's
inputs), so every workgroup of the resident grid runs at least two items: the prefetched operand
registers and the backward's prefetched P strip are consumed.
LayerNorm (rows, d), L lanes per row = 8 for d <= 32, 16 for d <= 64, 32 for d <= 128, 64 above:
    L = 8: (1, 4), (7, 20), (67, 32);  L = 16: (5, 36), (67, 64);  L = 32: (3, 68), (67, 128);
    L = 64: (2, 132), (67, 256);  scalar kernels: (7, 6), (9, 50), (5, 255) (d % 4) and (67, 64) with
    one operand 4 bytes off;  forward grid clamp 16 * num_cus: (128 * 16 * num_cus + 77, 4), which is
    also over the backward's kLnBlocks = 2048;  backward only: (260, 256) = 65 workgroups, 2 chunks of
    partials with 1 in the second, and (70001, 8) = 2188 workgroups asked for, clamped to 2048.
Small kernels: bst_pool's float4 kernel at d = 4 (G = 256), 12 (G = 85, one idle thread), 1024 (G = 1),
its scalar kernel at d = 6, 1028 and at a misaligned input; bst_pos_backward at B = 1, 63 (B <
kPosChunks), 64, 65 (per = 2: chunks 33.. empty), 130; bst_leaky_dropout's float4 kernel at n = 4, 1028
and its scalar kernel at n = 1, 1027 and a misaligned n = 1028."""
import functools

import pytest
import torch

import bst_train_ref as R
from rankops import _lib, ops
from test_gpu_train_ops import SENT, Flat, Guard, all_zero, close, invalid, rng_slot

pytestmark = pytest.mark.gpu

REL = {"att": 5e-5, "ln_fwd": 2.4e-5, "ln_fwd_big": 2.7e-4, "ln_bwd": 2.7e-5, "ln_bwd_big": 5.6e-5, "pos": 1.6e-5,
       "pool": 1.7e-5, "leaky": 9e-6}
f64 = torch.float64
SEED = 4242


def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def refused(code, fn, *a):
    with pytest.raises(_lib.RankOpsError) as e:
        fn(*a)
    assert e.value.code == code


def untouched(*bufs):
    for b in bufs:
        b.check("refused call")
        assert bool((b.v == SENT).all())


def engine_mask(slot, rows, d, p):
    return ops.dropout_mask(SEED, slot, rows, d, p) if p else None


def cpu(t):
    return None if t is None else t.cpu()


# ------------------------------------------------------------------ attention

@functools.lru_cache(maxsize=1)
def att_want(case):
    """The case's inputs and float64 oracle, computed once for its forward and its backward."""
    rc = R.att_resolve(case, num_cus())
    i = R.att_inputs(rc)
    return rc, i, R.att_eval(rc, i, f64)


def att_forward(case):
    (B, T, d, h), i, want = att_want(case)
    rel, lens = REL["att"], i.lens.cuda()
    qkv, P, ctx = Flat(B * T, 3 * d, fill=i.qkv), Flat(B, h, T, T), Flat(B * T, d)
    ops.bst_attn_train_forward(qkv.v, B, T, d, h, lens, P.v, ctx.v)
    close("P", P.check("P"), want["P"], rel)
    close("ctx", ctx.check("ctx"), want["ctx"], rel)
    qkv.check("qkv")
    masked = (torch.arange(T)[None, :] >= i.lens[:, None])[:, None, None, :].expand(B, h, T, T)
    assert all_zero(P.v.cpu()[masked])
    close("rows of P", P.v.sum(-1), torch.ones(B, h, T, dtype=f64), rel)
    ctx2 = Flat(B * T, d)
    if R.att_slots(T, d // h):  # the persistent kernels: the backward may recompute P
        ops.bst_attn_train_forward(qkv.v, B, T, d, h, lens, None, ctx2.v)
        assert torch.equal(ctx2.check("ctx without P"), ctx.v)
    else:
        refused(_lib.RK_ERR_UNSUPPORTED, ops.bst_attn_train_forward, qkv.v, B, T, d, h, lens, None, ctx2.v)
        untouched(ctx2)
    assert _lib.error_flags() == 0


def att_backward(case):
    """Fed the oracle's P rounded to fp32 and a seeded dctx: independent of the forward kernel."""
    (B, T, d, h), i, want = att_want(case)
    Bb = R.loop_batch(T, d, h, num_cus(), True) if case[0] == R.LOOP else B
    assert Bb <= B
    M, rel = Bb * T, REL["att"]
    qkv, dqkv = Flat(M, 3 * d, fill=i.qkv[:M]), Flat(M, 3 * d)
    P, dctx = want["P"][:Bb].float().contiguous().cuda(), i.dctx[:M].cuda()
    ops.bst_attn_train_backward(qkv.v, P, dctx, Bb, T, d, h, dqkv.v)
    got = dqkv.check("dqkv")  # overwritten: it started as the sentinel
    qkv.check("qkv")
    for k, n in enumerate(("dq", "dk", "dv")):
        close(n, got[:, k * d:(k + 1) * d].contiguous(), want[n][:M], rel)
    past = (torch.arange(T)[None, :] >= i.lens[:Bb, None]).reshape(M)
    assert all_zero(got.cpu()[past][:, d:])  # dK and dV rows of masked keys
    close("dbk", got[:, d:2 * d].sum(0), want["dk"][:M].sum(0), rel, R.dbk_scale(want["in:ds"][:Bb], want["in:q"][:Bb]))
    assert _lib.error_flags() == 0


@pytest.mark.parametrize("direction", ["forward", "backward"])  # varies fastest: one oracle per case
@pytest.mark.parametrize("case", R.ATT_CASES, ids=R.att_id)
def test_attention(case, direction):
    (att_forward if direction == "forward" else att_backward)(case)


def test_attention_refuses_shapes_past_its_envelope_and_takes_an_empty_batch():
    for B, T, d, h in ((2, 65, 8, 2), (2, 4, 65, 1)):
        qkv, dctx = torch.zeros(B * T, 3 * d, device="cuda"), torch.zeros(B * T, d, device="cuda")
        lens = torch.ones(B, dtype=torch.int64, device="cuda")
        P, ctx, dqkv = Flat(B, h, T, T), Flat(B * T, d), Flat(B * T, 3 * d)
        refused(_lib.RK_ERR_UNSUPPORTED, ops.bst_attn_train_forward, qkv, B, T, d, h, lens, P.v, ctx.v)
        refused(_lib.RK_ERR_UNSUPPORTED, ops.bst_attn_train_backward, qkv, P.v, dctx, B, T, d, h, dqkv.v)
        untouched(P, ctx, dqkv)
    B, T, d, h = 2, 4, 16, 4
    qkv, dctx = torch.zeros(B * T, 3 * d, device="cuda"), torch.zeros(B * T, d, device="cuda")
    lens = torch.ones(B, dtype=torch.int64, device="cuda")
    P, ctx, dqkv = Flat(B, h, T, T), Flat(B * T, d), Flat(B * T, 3 * d)
    ops.bst_attn_train_forward(qkv, 0, T, d, h, lens, P.v, ctx.v)
    ops.bst_attn_train_backward(qkv, P.v, dctx, 0, T, d, h, dqkv.v)
    untouched(P, ctx, dqkv)
    assert _lib.error_flags() == 0


# ------------------------------------------------------------------ residual + dropout + LayerNorm

LN_RUNS = [(c, False) for c in R.LN_CASES] + [(R.LN_MISALIGNED, True)]


def ln_id(run):
    (rows, d), mis = run
    return f"{rows}x{d}" + ("-misaligned" if mis else "")


def ln_module(i, d):
    ln = torch.nn.LayerNorm(d, eps=R.LN_EPS).cuda()
    with torch.no_grad():
        ln.weight.copy_(i.gamma)
        ln.bias.copy_(i.beta)
    return ln


def run_ln_forward(rc, i, p, slot, misaligned, base=None, o=None):
    rows, d = rc
    base = Flat(rows, d, fill=i.base if base is None else base)
    o = Flat(rows, d, offset=1 if misaligned else 0, fill=i.o if o is None else o)
    assert o.v.data_ptr() % 16 == (4 if misaligned else 0)
    r, y, mean, rstd = Flat(rows, d), Flat(rows, d), Flat(rows), Flat(rows)
    ops.bst_res_dropout_ln_forward(base.v, o.v, p, SEED, slot if p else None, ln_module(i, d), r.v, y.v, mean.v, rstd.v)
    base.check("base")
    o.check("o")
    return dict(r=r.check("r"), y=y.check("y"), mean=mean.check("mean"), rstd=rstd.check("rstd"))


@pytest.mark.parametrize("p", R.LN_PS)
@pytest.mark.parametrize("run", LN_RUNS, ids=ln_id)
def test_res_dropout_ln_forward(run, p):
    case, misaligned = run
    rc = rows, d = R.ln_resolve(case, num_cus())
    i = R.ln_inputs(rc)
    _, slot = rng_slot()
    mask = engine_mask(slot, rows, d, p)
    got, want = run_ln_forward(rc, i, p, slot, misaligned), R.ln_fwd_eval(rc, i, f64, cpu(mask))
    for n in ("r", "y", "mean", "rstd"):
        close(n, got[n], want[n], REL[R.ln_family(case, False)])
    if mask is not None:  # r = base exactly where the branch is dropped
        drop = mask == 0
        assert torch.equal(got["r"][drop].cpu(), i.base[drop.cpu()])
    assert _lib.error_flags() == 0


@pytest.mark.parametrize("run", LN_RUNS, ids=ln_id)
def test_res_dropout_ln_forward_of_constant_rows(run):
    """base + o = 0.5 in every column: mean = 0.5 and the variance 0 exactly, so y = beta bit for bit
    (as F.layer_norm gives) and rstd = 1 / sqrt(eps)."""
    case, misaligned = run
    rc = rows, d = R.ln_resolve(case, num_cus())
    i = R.ln_inputs(rc)
    quarter = torch.full((rows, d), 0.25)
    got = run_ln_forward(rc, i, 0.0, None, misaligned, base=quarter, o=quarter)
    assert bool((got["r"] == 0.5).all()) and bool((got["mean"] == 0.5).all())
    assert torch.equal(got["y"].cpu(), i.beta.expand(rows, d))
    close("rstd", got["rstd"], torch.full((rows,), R.LN_EPS, dtype=f64).rsqrt(), REL["ln_fwd"])


def test_res_dropout_ln_forward_float4_and_scalar_kernels_agree():
    rc = rows, d = R.LN_MISALIGNED
    i = R.ln_inputs(rc)
    _, slot = rng_slot()
    aligned, shifted = run_ln_forward(rc, i, 0.1, slot, False), run_ln_forward(rc, i, 0.1, slot, True)
    for n in ("r", "y", "mean", "rstd"):
        close(n + " (scalar against float4)", shifted[n], aligned[n].double().cpu(), REL["ln_fwd"])


def test_res_dropout_ln_forward_refuses_bad_arguments():
    _, slot = rng_slot()
    for d, p in ((257, 0.0), (8, 1.0)):
        rows = 3
        z = torch.zeros(rows, d, device="cuda")
        r, y, mean, rstd = Flat(rows, d), Flat(rows, d), Flat(rows), Flat(rows)
        ln = torch.nn.LayerNorm(d).cuda()
        invalid(ops.bst_res_dropout_ln_forward, z, z, p, SEED, slot, ln, r.v, y.v, mean.v, rstd.v)
        untouched(r, y, mean, rstd)


# ------------------------------------------------------------------ LayerNorm backward

def run_ln_backward(rc, i, p, slot, want, misaligned=False, with_d_o=True):
    rows, d = rc
    dy = Flat(rows, d, offset=1 if misaligned else 0, fill=i.dy)
    r, mean, rstd = want["in:r"].cuda(), want["in:mean"].cuda(), want["in:rstd"].cuda()
    dr, d_o, dgamma, dbeta = Flat(rows, d), Flat(rows, d), Flat(d), Flat(d)
    ops.bst_ln_backward(dy.v, r, mean, rstd, ln_module(i, d), p, SEED, slot if p else None, dr.v,
                        d_o.v if with_d_o else None, dgamma.v, dbeta.v)
    dy.check("dy")
    if not with_d_o:
        untouched(d_o)
    return dict(dr=dr.check("dr"), d_o=d_o.check("d_o"), dgamma=dgamma.check("dgamma"), dbeta=dbeta.check("dbeta"))


@pytest.mark.parametrize("p", R.LN_PS)
@pytest.mark.parametrize("run", LN_RUNS + [(c, False) for c in R.LN_BWD_EXTRA], ids=ln_id)
def test_ln_backward(run, p):
    case, misaligned = run
    rc = rows, d = R.ln_resolve(case, num_cus())
    i = R.ln_inputs(rc)
    _, slot = rng_slot()
    mask = engine_mask(slot, rows, d, p)
    want = R.ln_bwd_eval(rc, i, f64, cpu(mask))
    got = run_ln_backward(rc, i, p, slot, want, misaligned)
    for n in ("dr", "d_o", "dgamma", "dbeta"):
        close(n, got[n], want[n], REL[R.ln_family(case, True)])
    if mask is not None:
        assert all_zero(got["d_o"][mask == 0])
    again = run_ln_backward(rc, i, p, slot, want, misaligned)  # the parameter reduction is deterministic
    without = run_ln_backward(rc, i, p, slot, want, misaligned, with_d_o=False)
    for n in ("dr", "dgamma", "dbeta"):
        assert torch.equal(again[n], got[n]), f"{n}: two runs differ"
        assert torch.equal(without[n], got[n]), f"{n}: differs without d_o"
    assert _lib.error_flags() == 0


@pytest.mark.parametrize("case", R.POOL_LN_CASES, ids=str)
def test_pool_ln_backward(case):
    B, T, d, mean_pool = case
    rows, p = B * T, 0.1
    i = R.pool_ln_inputs(case)
    _, slot = rng_slot()
    mask = engine_mask(slot, rows, d, p)
    want = R.pool_ln_eval(case, i, f64, cpu(mask))
    ln, drow, lens = ln_module(i, d), i.drow.cuda(), i.lens.cuda()
    r, mean, rstd = want["in:r"].cuda(), want["in:mean"].cuda(), want["in:rstd"].cuda()
    out = [Flat(rows, d), Flat(rows, d), Flat(d), Flat(d)]
    assert ops.bst_pool_ln_backward(drow, R.POOL_COL, T, lens, mean_pool, r, mean, rstd, ln, p, SEED, slot,
                                    *(f.v for f in out)) is True
    for n, f in zip(("dr", "d_o", "dgamma", "dbeta"), out):
        close(n, f.check(n), want[n], REL["ln_bwd"])
    if not mean_pool:  # the unfused path train.py falls back to: bit-identical
        dx, two = Flat(rows, d), [Flat(rows, d), Flat(rows, d), Flat(d), Flat(d)]
        ops.bst_pool_backward(drow, R.POOL_COL, B, T, d, lens, False, dx.v)
        ops.bst_ln_backward(dx.check("dx"), r, mean, rstd, ln, p, SEED, slot, *(f.v for f in two))
        for n, f, g in zip(("dr", "d_o", "dgamma", "dbeta"), out, two):
            assert torch.equal(f.v, g.check(n)), f"{n}: fused and unfused differ"
    assert _lib.error_flags() == 0


@pytest.mark.parametrize("d,misaligned", [(6, False), (8, True)], ids=["d6", "misaligned_dr"])
def test_pool_ln_backward_says_when_it_does_not_apply(d, misaligned):
    B, T = 3, 5
    rows = B * T
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    lens = torch.ones(B, dtype=torch.int64, device="cuda")
    dr = Flat(rows, d, offset=1 if misaligned else 0)
    d_o, dgamma, dbeta = Flat(rows, d), Flat(d), Flat(d)
    assert ops.bst_pool_ln_backward(z(B, d + 5), R.POOL_COL, T, lens, False, z(rows, d), z(rows), z(rows),
                                    torch.nn.LayerNorm(d).cuda(), 0.0, SEED, None, dr.v, d_o.v, dgamma.v,
                                    dbeta.v) is False
    untouched(dr, d_o, dgamma, dbeta)


# ------------------------------------------------------------------ small kernels

@pytest.mark.parametrize("case", R.ADD_POS_CASES, ids=str)
def test_add_pos(case):
    rows, T, d = case
    assert (rows * d) % 256 and rows % T
    i = R.add_pos_inputs(case)
    x, xp = Flat(rows, d, fill=i.x), Flat(rows, d)
    ops.bst_add_pos(x.v, i.pos.cuda(), T, xp.v)
    close("xp", xp.check("xp"), R.add_pos_eval(case, i, f64)["xp"], REL["pos"])
    assert torch.equal(xp.v.cpu(), R.add_pos(i.x, i.pos, T))  # one IEEE add
    x.check("x")


@pytest.mark.parametrize("case", R.GATHER_CASES, ids=str)
def test_gather_pos(case):
    rows, T, d = case
    i = R.add_pos_inputs(case)
    table, pos = i.table.cuda()[:, :d], i.pos.cuda()
    assert table.stride(0) == d + 4
    assert _lib.error_flags() == 0
    for oob in (False, True):
        idx = i.idx.clone()
        if oob:
            idx[1], idx[-1] = -1, R.GATHER_VOCAB
        x, xp = Flat(rows, d), Flat(rows, d)
        assert ops.bst_gather_pos(table, idx.cuda(), T, pos, x.v, xp.v) is True
        wx, wxp = R.gather_pos(i.table[:, :d].double(), idx, i.pos.double(), T)
        assert torch.equal(x.check("x").cpu(), wx.float())
        close("xp", xp.check("xp"), wxp, REL["pos"])
        if oob:
            bad = torch.tensor([1, rows - 1])
            assert all_zero(x.v.cpu()[bad]) and torch.equal(xp.v.cpu()[bad], i.pos[bad % T])
        flags = _lib.error_flags()
        assert (flags != 0 and flags & _lib.RK_FLAG_INDEX_OOB) if oob else flags == 0
    assert _lib.error_flags() == 0  # reading the flags reset them


def test_gather_pos_says_when_it_does_not_apply():
    rows, T, d = 5, 3, 6
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    x, xp = Flat(rows, d), Flat(rows, d)
    idx = torch.zeros(rows, dtype=torch.int64, device="cuda")
    assert ops.bst_gather_pos(z(4, d), idx, T, z(T, d), x.v, xp.v) is False
    untouched(x, xp)


@pytest.mark.parametrize("case", R.POOL_CASES, ids=str)
def test_pool(case):
    B, T, d, mean, misaligned = case
    i = R.pool_inputs(case)
    x = Flat(B * T, d, offset=1 if misaligned else 0, fill=i.x)
    row = Guard(B, d, c0=R.POOL_COL, pad=2)
    ops.bst_pool(x.v, B, T, i.lens.cuda(), mean, row.buf[:B], R.POOL_COL)
    close("row", row.check("row"), R.pool_eval(case, i, f64)["row"], REL["pool"])
    x.check("x")
    assert _lib.error_flags() == 0


@pytest.mark.parametrize("case", R.POOL_BWD_CASES, ids=str)
def test_pool_backward(case):
    B, T, d, mean = case
    i = R.pool_inputs(case)
    dx = Flat(B * T, d)
    ops.bst_pool_backward(i.drow.cuda(), R.POOL_COL, B, T, d, i.lens.cuda(), mean, dx.v)
    close("dx", dx.check("dx"), R.pool_bwd_eval(case, i, f64)["dx"], REL["pool"])


@pytest.mark.parametrize("case", R.POS_BWD_CASES, ids=str)
def test_pos_backward_accumulates(case):
    B, (T, d) = case
    i = R.pos_bwd_inputs(case)
    dpos = Flat(T + 1, d, fill=i.dpos0)  # a table one row longer than T: that row stays
    ops.bst_pos_backward(i.dxp.cuda(), B, T, dpos.v)
    close("dpos", dpos.check("dpos"), R.pos_bwd_eval(case, i, f64)["dpos"], REL["pos"])
    assert torch.equal(dpos.v[T].cpu(), i.dpos0[T])


@pytest.mark.parametrize("case", R.LEAKY_CASES, ids=str)
def test_leaky_dropout_forward_backward(case):
    n, misaligned, p = case
    i = R.leaky_inputs(case)
    _, slot = rng_slot()
    mask = engine_mask(slot, 1, n, p)
    mask = None if mask is None else mask.view(n)
    f = Flat(n, offset=1 if misaligned else 0, fill=i.f)
    assert f.v.data_ptr() % 16 == (4 if misaligned else 0)
    a, df, da = Flat(n), Flat(n), i.da.cuda()
    ops.bst_leaky_dropout(None, f.v, R.SLOPE, p, SEED, slot if p else None, False, a.v)
    ops.bst_leaky_dropout(da, f.v, R.SLOPE, p, SEED, slot if p else None, True, df.v)
    want = R.leaky_eval(case, i, f64, cpu(mask))
    close("a", a.check("a"), want["a"], REL["leaky"])
    close("df", df.check("df"), want["df"], REL["leaky"])
    f.check("f")
    if mask is not None:
        assert all_zero(a.v[mask == 0]) and all_zero(df.v[mask == 0])
    out = Flat(n)
    invalid(ops.bst_leaky_dropout, None, f.v, R.SLOPE, p, SEED, slot if p else None, True, out.v)
    untouched(out)
    assert _lib.error_flags() == 0
