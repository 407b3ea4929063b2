"""Plain torch restatement of the BST training operations (csrc/train_bst.hip), one small function per
operation, written as the mathematics of each kernel's header comment so that torch.autograd
differentiates it.  It runs in the dtype of its inputs: float64 is the oracle of
tests/test_gpu_bst_train_ops.py, and the same code in float32 gives the drift its tolerances rest on
(tests/test_bst_train_ref.py).  Dropout is a multiplier mask (0 or 1 / (1 - p)) handed in by the
caller: the GPU tests take it from the engine (ops.dropout_mask), the CPU tests draw one.

The second half is the case table both test files share: the shapes, seeded inputs and one `*_eval`
function per operation family that returns every compared tensor in the requested dtype.  Keys with a
colon are not compared: "scale:<name>" is the scale of <name>'s summands (a tensor that is zero in
exact arithmetic), "in:<name>" an input the GPU test feeds to the kernel."""
import itertools
import math
from types import SimpleNamespace as NS

import torch

from train_ops_ref import MARGIN, _grads, _leaf, gen, rel_err  # noqa: F401  (shared with the GPU file)

LN_EPS = 1e-5
SLOPE = 0.01
NUM_CUS = 256      # MI355X; the GPU file resolves the looping cases with the device's own count
WG_PER_CU = 8      # the most 256-thread workgroups a CU holds
LDS_PER_CU = 160 * 1024


# ------------------------------------------------------------------ operations

def add_pos(x, pos, T):
    """x (M, d), pos (>= T, d): xp[m] = x[m] + pos[m % T]."""
    M = x.shape[0]  # (repeat, not an index: its gradient is a plain sum in a fixed order)
    return x + pos[:T].repeat(-(-M // T), 1)[:M]


def gather_pos(table, idx, pos, T):
    """x[m] = table[idx[m]] (an out-of-range index: a zero row), xp = add_pos(x)."""
    ok = (idx >= 0) & (idx < table.shape[0])
    x = table[idx.clamp(0, table.shape[0] - 1)] * ok[:, None].to(table.dtype)
    return x, add_pos(x, pos, T)


def attention(qkv, B, T, d, heads, seq_len, delta=None):
    """qkv (B*T, 3d) = [Q | K | V]: P = softmax(mask(Q K^T / sqrt(dh)) (+ delta)) (B, h, T, T), keys
    j >= seq_len[b] masked with -inf; ctx = P V (B*T, d)."""
    dh = d // heads
    q, k, v = (qkv[:, c * d:(c + 1) * d].reshape(B, T, heads, dh).transpose(1, 2) for c in range(3))
    s = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(dh)
    if delta is not None:
        s = s + delta
    masked = torch.arange(T)[None, :] >= seq_len[:, None]
    P = torch.softmax(s.masked_fill(masked[:, None, None, :], float("-inf")), dim=-1)
    return P, torch.matmul(P, v).transpose(1, 2).reshape(B * T, d)


def res_dropout_ln(base, o, mask, gamma, beta, eps):
    """r = base + mask * o; y = LayerNorm(r) with the biased variance: r, y, mean, rstd."""
    r = base + (o if mask is None else o * mask)
    mean = r.sum(1) / r.shape[1]
    rc = r - mean[:, None]
    rstd = 1.0 / torch.sqrt((rc * rc).sum(1) / r.shape[1] + eps)
    return r, rc * rstd[:, None] * gamma + beta, mean, rstd


def ln_backward(dy, r, mean, rstd, gamma, mask):
    """From the saved r, mean, rstd: dr = rstd (g - mean(g) - xhat mean(g xhat)) with g = dy gamma;
    d_o = mask * dr; dgamma = sum dy xhat; dbeta = sum dy."""
    xh = (r - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    dr = rstd[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return dr, (dr if mask is None else dr * mask), (dy * xh).sum(0), dy.sum(0)


def pool(x, B, T, seq_len, mean):
    """x (B*T, d) -> (B, d): the sum over all T rows, or that sum / seq_len."""
    s = x.reshape(B, T, -1).sum(1)
    return s / seq_len[:, None].to(x.dtype) if mean else s


def pool_backward(drow, T, seq_len, mean):
    """The broadcast of drow (B, d) to (B*T, d) (/ seq_len for mean pooling)."""
    g = drow / seq_len[:, None].to(drow.dtype) if mean else drow
    return g[:, None, :].expand(-1, T, -1).reshape(drow.shape[0] * T, -1)


def pool_ln_backward(drow, T, seq_len, mean_pool, r, mean, rstd, gamma, mask):
    return ln_backward(pool_backward(drow, T, seq_len, mean_pool), r, mean, rstd, gamma, mask)


def leaky_dropout(f, mask, slope):
    """a = mask * (f > 0 ? f : slope f); at f = +-0 the slope side, as the kernel's `f > 0`."""
    a = torch.where(f > 0, f, f * slope)
    return a if mask is None else a * mask


def leaky_dropout_backward(da, f, mask, slope):
    df = da * torch.where(f > 0, torch.ones_like(f), torch.full_like(f, slope))
    return df if mask is None else df * mask


def pos_backward(dxp, B, T, dpos0):
    """dpos0[t] + sum_b dxp[b T + t]."""
    return dpos0 + dxp.reshape(B, T, -1).sum(0)


# ------------------------------------------------------------------ the case table

def cpu_mask(g, shape, p):
    """A multiplier mask as the engine makes them, drawn on the CPU (the drift measurement)."""
    if not p:
        return None
    return (torch.rand(*shape, generator=g) >= p).float() * float(torch.tensor(1.0 / (1.0 - p)).float())


def pad16(v):
    return (v + 15) & ~15


def att_lds_bytes(T, dh, bwd):
    """att_lds_bytes of train_bst.hip: [TP][DP + 4] operand tiles, in the backward also P and dS."""
    TP, DP = pad16(T), pad16(dh)
    return 4 * (4 * TP * (DP + 4) + 2 * TP * (TP + 4) if bwd else 3 * TP * (DP + 4))


def att_slots(T, dh):
    """att_slots of train_bst.hip (0: the one-item kernels, also taken when T % 4 != 0)."""
    if dh % 4 or T % 4:
        return 0
    n = pad16(T) * pad16(dh) // 4
    return 1 if n <= 256 else 2 if n <= 512 else 4


def loop_batch(T, d, heads, num_cus, bwd):
    """The smallest B with B * heads >= 2 * bound + 3, bound = num_cus * min(8, 160 KiB / lds): the
    persistent grid is at most `bound` workgroups whatever occupancy the runtime reports, so every
    workgroup runs at least 2 items (2 or 3 at that bound).  2 * bound + 3 is odd: with heads = 4 the
    item count is rounded up to the next multiple of heads."""
    bound = num_cus * min(WG_PER_CU, LDS_PER_CU // att_lds_bytes(T, d // heads, bwd))
    return -(-(2 * bound + 3) // heads)


LOOP = "loop"
# (B, T, d, heads); B = LOOP: loop_batch of the forward (the backward runs on the first
# loop_batch(bwd) samples of the same inputs)
ATT_CASES = [(3, 5, 6, 2), (2, 18, 8, 2), (3, 17, 12, 1), (2, 1, 4, 1), (LOOP, 4, 16, 4), (2, 20, 80, 2),
             (LOOP, 32, 64, 1), (2, 44, 104, 2), (LOOP, 64, 64, 1),
             (3, 8, 6, 2)]  # beyond the issue's table: one-item kernel, scalar staging with a float4 P (T % 4 == 0)


def att_id(c):
    return "-".join(str(v) for v in c)


def att_resolve(case, num_cus=NUM_CUS):
    B, T, d, heads = case
    return (loop_batch(T, d, heads, num_cus, False) if B == LOOP else B, T, d, heads)


def att_lens(B, T):
    """1, T and values between, across the 16-multiples where T allows."""
    cand = [1, T] + [v for v in (T // 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 2, 3) if 1 < v < T]
    return torch.tensor([cand[b % len(cand)] for b in range(B)], dtype=torch.int64)


def att_inputs(rcase):
    B, T, d, heads = rcase
    g = gen("bst_att", rcase)
    return NS(qkv=torch.randn(B * T, 3 * d, generator=g), dctx=torch.randn(B * T, d, generator=g), lens=att_lens(B, T))


def att_eval(rcase, i, dtype):
    """P, ctx, and the gradients of (ctx * dctx).sum() w.r.t. [Q | K | V].  dbk = sum over the rows of
    dK (the gradient of w_k's bias) is 0 in exact arithmetic: dK[j] = sum_i dS[i, j] Q[i] and the rows
    of a softmax's Jacobian sum to zero, so it is compared on the scale of its summands |dS| |Q|."""
    B, T, d, heads = rcase
    qkv = _leaf(i.qkv, dtype)
    delta = torch.zeros(B, heads, T, T, dtype=dtype, requires_grad=True)  # its gradient is sqrt(dh) dS
    P, ctx = attention(qkv, B, T, d, heads, i.lens, delta)
    dqkv, ds = _grads((ctx * i.dctx.to(dtype)).sum(), [qkv, delta])
    ds = ds / math.sqrt(d // heads)
    q = qkv.detach()[:, :d].reshape(B, T, heads, d // heads).transpose(1, 2)
    dk = dqkv[:, d:2 * d]
    return {"P": P.detach(), "ctx": ctx.detach(), "dq": dqkv[:, :d], "dk": dk, "dv": dqkv[:, 2 * d:],
            "dbk": dk.sum(0), "scale:dbk": dbk_scale(ds, q), "in:ds": ds, "in:q": q}


def dbk_scale(ds, q):
    """max over the columns of sum_{b, i, j} |dS[i, j]| |Q[i]|: the summands of dbk (ds, q: (B, h, T, .))."""
    return torch.einsum("bhij,bhic->hc", ds.abs(), q.abs()).max()


# (rows, d); rows = LOOP: the forward's 16 * num_cus grid clamp (ln_resolve)
LN_CASES = [(1, 4), (7, 20), (67, 32), (5, 36), (67, 64), (3, 68), (67, 128), (2, 132), (67, 256),  # L = 8 .. 64
            (7, 6), (9, 50), (5, 255),                                                                # scalar: d % 4
            (LOOP, 4)]
LN_BWD_EXTRA = [(260, 256), (70001, 8)]  # 65 workgroups = 2 chunks of partials; the 2048-workgroup clamp
LN_MISALIGNED = (67, 64)                 # run again with one operand 4 bytes off: the scalar kernels
LN_PS = (0.0, 0.1)


def ln_lanes(d):
    """ln_lanes of train_bst.hip for 16-B aligned pointers (0: the scalar kernels)."""
    if d % 4 or d > 256:
        return 0
    L = 8
    while 4 * L < d:
        L *= 2
    return L


def ln_resolve(case, num_cus=NUM_CUS):
    """LOOP: d = 4 holds 8 rows per wave and 4 row groups in flight, 128 rows per workgroup and step;
    one more than 16 * num_cus workgroups' worth of rows clamps the grid, and the 77 rows past it are
    the second step of the first workgroup's first wave and a part of its second."""
    rows, d = case
    return (128 * 16 * num_cus + 77 if rows == LOOP else rows, d)


def ln_family(case, bwd):
    """The half million rows of the grid-clamp case are a family of their own: the worst of so many
    rows of 4 columns (a small variance amplifies the rounding of r - mean) would set the tolerance of
    every other case."""
    return ("ln_bwd" if bwd else "ln_fwd") + ("_big" if case[0] == LOOP else "")


def ln_inputs(rcase):
    rows, d = rcase
    g = gen("bst_ln", rcase)
    return NS(base=torch.randn(rows, d, generator=g), o=torch.randn(rows, d, generator=g),
              gamma=1.0 + 0.5 * torch.randn(d, generator=g), beta=0.5 * torch.randn(d, generator=g),
              dy=torch.randn(rows, d, generator=g), cpu_mask=cpu_mask(g, (rows, d), 0.1))


def ln_fwd_eval(rcase, i, dtype, mask):
    t = lambda x: None if x is None else x.to(dtype)  # noqa: E731
    r, y, mean, rstd = res_dropout_ln(t(i.base), t(i.o), t(mask), t(i.gamma), t(i.beta), LN_EPS)
    return dict(r=r, y=y, mean=mean, rstd=rstd)


def ln_bwd_eval(rcase, i, dtype, mask, drow=None):
    """The backward from the float64 forward's r, mean, rstd rounded to float32 (what the kernel is
    fed).  drow = (drow (B, d), T, seq_len, mean_pool): the pooled-row form's incoming gradient."""
    f = ln_fwd_eval(rcase, i, torch.float64, mask)
    r, mean, rstd = f["r"].float(), f["mean"].float(), f["rstd"].float()
    t = lambda x: None if x is None else x.to(dtype)  # noqa: E731
    dy = t(i.dy) if drow is None else pool_backward(t(drow[0]), drow[1], drow[2], drow[3])
    dr, d_o, dgamma, dbeta = ln_backward(dy, t(r), t(mean), t(rstd), t(i.gamma), t(mask))
    return {"dr": dr, "d_o": d_o, "dgamma": dgamma, "dbeta": dbeta, "in:r": r, "in:mean": mean, "in:rstd": rstd}


# (B, T, d, mean pooling) of rk_bst_pool_ln_backward; rows = B * T
POOL_LN_CASES = [(3, T, d, mean) for T, d, mean in itertools.product((1, 5), (4, 36, 128), (False, True))]
POOL_COL = 3


def pool_ln_inputs(case):
    B, T, d, mean = case
    g = gen("bst_pool_ln", case)
    i = ln_inputs((B * T, d))
    i.drow = torch.randn(B, POOL_COL + d + 2, generator=g)
    i.lens = torch.randint(1, T + 1, (B,), generator=g)
    return i


def pool_ln_eval(case, i, dtype, mask):
    B, T, d, mean = case
    return ln_bwd_eval((B * T, d), i, dtype, mask, (i.drow[:, POOL_COL:POOL_COL + d], T, i.lens, mean))


ADD_POS_CASES = [(7, 5, 6), (13, 20, 20)]  # (rows, T, d): rows * d is no multiple of 256, rows none of T
GATHER_CASES = [(11, 5, 4), (13, 4, 20)]   # (rows of idx, T, d)
GATHER_VOCAB = 9


def add_pos_inputs(case):
    rows, T, d = case
    g = gen("bst_add_pos", case)
    return NS(x=torch.randn(rows, d, generator=g), pos=torch.randn(T + 1, d, generator=g),
              table=torch.randn(GATHER_VOCAB, d + 4, generator=g),  # a strided table: ld_table = d + 4
              idx=torch.randint(0, GATHER_VOCAB, (rows,), generator=g))


def add_pos_eval(case, i, dtype):
    rows, T, d = case
    x, xp = gather_pos(i.table[:, :d].to(dtype), i.idx, i.pos.to(dtype), T)
    return dict(xp=add_pos(i.x.to(dtype), i.pos.to(dtype), T), gather_xp=xp)


POS_BWD_CASES = list(itertools.product((1, 63, 64, 65, 130), ((5, 6), (20, 16))))  # (B, (T, d))


def pos_bwd_inputs(case):
    B, (T, d) = case
    g = gen("bst_pos_bwd", case)
    return NS(dxp=torch.randn(B * T, d, generator=g), dpos0=torch.randn(T + 1, d, generator=g))


def pos_bwd_eval(case, i, dtype):
    """Through autograd: dpos0 + the gradient of (add_pos(x, pos) * dxp).sum() w.r.t. pos (the row
    past T gets none)."""
    B, (T, d) = case
    pos = torch.zeros(T + 1, d, dtype=dtype, requires_grad=True)
    g, = _grads((add_pos(torch.zeros(B * T, d, dtype=dtype), pos, T) * i.dxp.to(dtype)).sum(), [pos])
    return dict(dpos=i.dpos0.to(dtype) + g)


# (B, T, d, mean, misaligned input): float4 at d in 4, 12, 1024; scalar at d in 6, 1028 and at a misaligned input
POOL_CASES = ([(3, T, d, mean, False) for d, T, mean in itertools.product((4, 12, 1024, 6, 1028), (1, 5, 70),
                                                                          (False, True))]
              + [(3, 5, 12, mean, True) for mean in (False, True)])
POOL_BWD_CASES = [(B, T, d, mean) for (B, T, d), mean in itertools.product(((1, 1, 1), (3, 5, 6), (2, 7, 36)),
                                                                         (False, True))]


def pool_inputs(case):
    B, T, d = case[:3]
    g = gen("bst_pool", case)
    return NS(x=torch.randn(B * T, d, generator=g), lens=torch.randint(1, T + 1, (B,), generator=g),
              drow=torch.randn(B, POOL_COL + d + 2, generator=g))


def pool_eval(case, i, dtype):
    B, T, d, mean = case[:4]
    return dict(row=pool(i.x.to(dtype), B, T, i.lens, mean))


def pool_bwd_eval(case, i, dtype):
    """Through autograd: the gradient of (pool(x) * drow).sum() w.r.t. x."""
    B, T, d, mean = case
    x = torch.zeros(B * T, d, dtype=dtype, requires_grad=True)
    dx, = _grads((pool(x, B, T, i.lens, mean) * i.drow[:, POOL_COL:POOL_COL + d].to(dtype)).sum(), [x])
    return dict(dx=dx)


# (n, misaligned, p): float4 at n in 4, 1028; scalar at n in 1, 1027 and at a misaligned n = 1028
LEAKY_CASES = [(n, mis, p) for (n, mis), p in itertools.product(((4, False), (1028, False), (1, False), (1027, False),
                                                                 (1028, True)), (0.0, 0.1))]
LEAKY_EXCLUDED = 0  # the sign of f is taken from the same fp32 f on both sides: every element is compared


def leaky_inputs(case):
    n, mis, p = case
    g = gen("bst_leaky", n, mis)
    i = NS(f=torch.randn(n, generator=g), da=torch.randn(n, generator=g), cpu_mask=cpu_mask(g, (n,), p))
    for k, v in enumerate((0.0, -0.0, -1.0, -0.5)[:n] if n >= 4 else (-0.0,)):
        i.f[(k * 7) % n] = v  # +0.0, -0.0 and exact negatives
    return i


def leaky_eval(case, i, dtype, mask):
    """a, and through autograd the gradient of (a * da).sum() w.r.t. f."""
    f = _leaf(i.f, dtype)
    a = leaky_dropout(f, None if mask is None else mask.to(dtype), SLOPE)
    df, = _grads((a * i.da.to(dtype)).sum(), [f])
    return dict(a=a.detach(), df=df)


def family_evals(num_cus=NUM_CUS):
    """family -> list of (case id, eval(dtype) -> dict of tensors): every case of the GPU file, with
    dropout masks drawn on the CPU."""
    fam = {k: [] for k in ("att", "ln_fwd", "ln_fwd_big", "ln_bwd", "ln_bwd_big", "pos", "pool", "leaky")}
    for c in ATT_CASES:
        rc = att_resolve(c, num_cus)
        i = att_inputs(rc)
        fam["att"].append((att_id(c), lambda dt, rc=rc, i=i: att_eval(rc, i, dt)))
    for c in LN_CASES + LN_BWD_EXTRA:
        rc = ln_resolve(c, num_cus)
        i = ln_inputs(rc)
        for p in LN_PS:
            m = i.cpu_mask if p else None
            if c in LN_CASES:
                fam[ln_family(c, False)].append((f"{c} p={p}", lambda dt, rc=rc, i=i, m=m: ln_fwd_eval(rc, i, dt, m)))
            fam[ln_family(c, True)].append((f"{c} p={p}", lambda dt, rc=rc, i=i, m=m: ln_bwd_eval(rc, i, dt, m)))
    for c in POOL_LN_CASES:
        i = pool_ln_inputs(c)
        fam["ln_bwd"].append((f"pooled {c}", lambda dt, c=c, i=i: pool_ln_eval(c, i, dt, i.cpu_mask)))
    for c in ADD_POS_CASES + GATHER_CASES:
        i = add_pos_inputs(c)
        fam["pos"].append((f"add_pos {c}", lambda dt, c=c, i=i: add_pos_eval(c, i, dt)))
    for c in POS_BWD_CASES:
        i = pos_bwd_inputs(c)
        fam["pos"].append((f"pos_backward {c}", lambda dt, c=c, i=i: pos_bwd_eval(c, i, dt)))
    for c in POOL_CASES:
        i = pool_inputs(c)
        fam["pool"].append((f"pool {c}", lambda dt, c=c, i=i: pool_eval(c, i, dt)))
    for c in POOL_BWD_CASES:
        i = pool_inputs(c)
        fam["pool"].append((f"pool_backward {c}", lambda dt, c=c, i=i: pool_bwd_eval(c, i, dt)))
    for c in LEAKY_CASES:
        i = leaky_inputs(c)
        fam["leaky"].append((str(c), lambda dt, c=c, i=i: leaky_eval(c, i, dt, i.cpu_mask)))
    return fam
