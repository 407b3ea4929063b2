"""Plain torch restatement of the train-mode tail, DIN attention and AFM attention operations
(csrc/train_bn.hip, train_din.hip, train_afm.hip), one small function per operation, written as the
mathematics of each kernel's header comment so that torch.autograd differentiates it.  It runs in
the dtype of its inputs: float64 is the oracle of tests/test_gpu_train_ops.py, and the same code in
float32 gives the drift its tolerances rest on (tests/test_train_ops_ref.py).

The second half is the case table both test files share: the shapes, seeded inputs and one `*_eval`
function per operation family that returns every compared tensor (forward outputs and the gradients
of a seeded scalar loss) in the requested dtype."""
import hashlib
import itertools
import math
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

NO_BN = "no batch norm"        # bn_act's gamma: no BatchNorm at all (gamma None: BatchNorm without affine)
MASK_SCORE = float(-2 ** 32 + 1)
MARGIN = 50.0                  # GPU tolerance / CPU fp32 drift (test_gpu_dien.py's margin)
NEAR_ZERO = 1e-5               # |u| < NEAR_ZERO * max|u|: the sign of u may differ between fp32 and fp64


# ------------------------------------------------------------------ operations

def batch_stats(x):
    """mean, biased variance, unbiased variance over the rows (B = 1: the biased one, 0, for both)."""
    B = x.shape[0]
    mean = x.sum(0) / B
    xc = x - mean
    var = (xc * xc).sum(0) / B
    return mean, var, (var * B / (B - 1) if B > 1 else var)


def bn_pre(z, bias, gamma, beta, eps):
    """The pre-activation u of bn_act and the batch statistics (None without BN)."""
    x = z if bias is None else z + bias
    if isinstance(gamma, str) and gamma == NO_BN:
        return x, None, None, None, None
    mean, var, unbiased = batch_stats(x)
    invstd = 1.0 / torch.sqrt(var + eps)
    u = (x - mean) * invstd
    if gamma is not None:
        u = u * gamma
    if beta is not None:
        u = u + beta
    return u, mean, invstd, var, unbiased


def bn_act(z, bias, gamma, beta, eps, act, slope, mask):
    """y = mask * act(gamma * (z + bias - mean) * invstd + beta); act in none / relu / leaky."""
    u, mean, invstd, var, unbiased = bn_pre(z, bias, gamma, beta, eps)
    if act == "relu":
        u = torch.relu(u)
    elif act == "leaky":
        u = F.leaky_relu(u, slope)
    elif act != "none":
        raise ValueError(act)
    if mask is not None:
        u = u * mask
    return u, mean, invstd, var, unbiased


def dice(z, bias, alpha, eps):
    """Dice in train mode: p = sigmoid(BatchNorm(affine=False)(x)), y = alpha (1 - p) x + p x."""
    x = z if bias is None else z + bias
    mean, var, unbiased = batch_stats(x)
    invstd = 1.0 / torch.sqrt(var + eps)
    p = torch.sigmoid((x - mean) * invstd)
    return alpha * (1.0 - p) * x + p * x, mean, invstd, var, unbiased


def prelu(z, bias, weight):
    """x > 0 ? x : weight * x with one weight or one per column."""
    x = z if bias is None else z + bias
    return torch.where(x > 0, x, weight * x)


def din_pool(a2, w3, b3, keys, lens, softmax):
    """a2 (B, T, A2), keys (B, T, H): scores -> masked (softmax) weights -> weighted key sum."""
    B, T, H = keys.shape
    s = (a2 * w3).sum(-1) + b3
    mask = torch.arange(T)[None, :] < lens[:, None]
    if softmax:
        s = torch.where(mask, s, torch.full_like(s, MASK_SCORE)) / (H ** 0.5)
        w = torch.softmax(s, dim=1)
    else:
        w = s.masked_fill(~mask, 0.0)
    return w, (w.unsqueeze(2) * keys).sum(1)


def din_cross(q, k):
    qe = q.unsqueeze(1).expand_as(k)
    return torch.cat([qe, k, qe - k, qe * k], dim=2)


def row_l2(v, scale):
    return scale * torch.linalg.vector_norm(v, dim=1).sum()


def afm_pairs(e):
    """e (B, F, D) -> (B, P, D), e_i * e_j for i < j, i-major."""
    i, j = torch.triu_indices(e.shape[1], e.shape[1], offset=1)
    return e[:, i] * e[:, j]


def afm_pool(a1, w2, b2, pairs, dense, wd, bd, wp, bp):
    """a1 (B, P, A), pairs (B, P, D), dense (B, nd) -> weights (B, P), ws (B, D), logit (B), pred (B)."""
    s = (a1 * w2).sum(-1) + b2
    w = torch.softmax(s, dim=1)
    ws = (w.unsqueeze(2) * pairs).sum(1)
    logit = ((dense * wd).sum(1) + bd) + ((ws * wp).sum(1) + bp)
    return w, ws, logit, torch.sigmoid(logit)


def fm_second(e):
    """DeepFM's second-order term of e (B, F, D): 0.5 sum_d ((sum_f e)^2 - sum_f e^2)."""
    s = e.sum(1)
    return 0.5 * (s * s - (e * e).sum(1)).sum(1)


def fm_combine(fm1, fm2, deep, w, b):
    """final_layer (Linear(3, 1) over [fm1, fm2, deep]) + sigmoid: total, prob."""
    total = w[0] * fm1 + w[1] * fm2 + w[2] * deep + b
    return total, torch.sigmoid(total)


# ------------------------------------------------------------------ the case table

def gen(*key):
    g = torch.Generator()
    g.manual_seed(int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:6], "little"))
    return g


def _grads(loss, leaves):
    got = torch.autograd.grad(loss, leaves, allow_unused=True)
    return [torch.zeros_like(l) if g is None else g for g, l in zip(got, leaves)]


def _leaf(t, dtype):
    return t.to(dtype).requires_grad_(True)


def near_zero(u):
    return u.abs() < NEAR_ZERO * u.abs().max()


BN_SHAPES = [(1, 7), (3, 64), (5, 65), (63, 1), (65, 130), (130, 64)]
ACTS = [("none", 0.0), ("relu", 0.0), ("leaky", 0.01)]
# (B, N, bn, act, slope, p, bias); the cases with a bias run on column slices of wider buffers
BN_CASES = [(B, N, bn, act, slope, p, bias) for (B, N), bn, (act, slope), p, bias
            in itertools.product(BN_SHAPES, (True, False), ACTS, (0.0, 0.25), (True, False))]
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def bn_id(c):
    B, N, bn, act, slope, p, bias = c
    return f"{B}x{N}-{'bn' if bn else 'nobn'}-{act}-p{p}-{'bias' if bias else 'nobias'}"


def bn_inputs(case):
    """Seeded fp32 inputs.  With BN the seed is advanced until no fp64 pre-activation is near zero
    (near_zero), so every element of y and dz is compared; without BN a few z + bias are exact zeros."""
    B, N, bn, act, slope, p, bias = case
    for attempt in range(64):
        g = gen("bn", case, attempt)
        i = NS(z=torch.randn(B, N, generator=g), bias=torch.randn(N, generator=g) if bias else None,
               gamma=1.0 + 0.5 * torch.randn(N, generator=g), beta=0.5 * torch.randn(N, generator=g),
               running_mean=torch.randn(N, generator=g), running_var=0.5 + torch.rand(N, generator=g),
               G=torch.randn(B, N, generator=g))
        i.cpu_mask = ((torch.rand(B, N, generator=g) >= p).float() * float(torch.tensor(1.0 / (1.0 - p)).float())
                      if p > 0 else None)
        if not bn:
            for k in range(min(3, B * N)):  # exact zeros of z + bias: relu' = 0, leaky' = slope on both sides
                b, n = (k * 7) % B, (k * 11) % N
                i.z[b, n] = -i.bias[n] if bias else 0.0
            return i
        u = bn_pre(i.z.double(), None if i.bias is None else i.bias.double(), i.gamma.double(), i.beta.double(),
                   BN_EPS)[0]
        if not bool(near_zero(u).any()):
            return i
    raise AssertionError(f"no seed keeps the pre-activations of {case} away from zero")


def bn_eval(case, i, dtype, mask):
    B, N, bn, act, slope, p, bias = case
    z = _leaf(i.z, dtype)
    gamma, beta = (_leaf(i.gamma, dtype), _leaf(i.beta, dtype)) if bn else (NO_BN, None)
    y, mean, invstd, var, unbiased = bn_act(z, None if i.bias is None else i.bias.to(dtype), gamma, beta, BN_EPS, act,
                                            slope, None if mask is None else mask.to(dtype))
    out = {"y": y.detach()}
    grads = _grads((y * i.G.to(dtype)).sum(), [z] + ([gamma, beta] if bn else []))
    out["dz"] = grads[0]
    if bn:
        out.update(save_mean=mean.detach(), save_invstd=invstd.detach(), dgamma=grads[1], dbeta=grads[2],
                   running_mean=BN_MOMENTUM * mean.detach() + (1 - BN_MOMENTUM) * i.running_mean.to(dtype),
                   running_var=BN_MOMENTUM * unbiased.detach() + (1 - BN_MOMENTUM) * i.running_var.to(dtype))
    return out


DICE_CASES = [(B, N, bias) for (B, N), bias in itertools.product(BN_SHAPES, (True, False))]


def dice_inputs(case):
    B, N, bias = case
    g = gen("dice", case)
    i = NS(z=torch.randn(B, N, generator=g), bias=torch.randn(N, generator=g) if bias else None,
           alpha=torch.randn(N, generator=g), running_mean=torch.randn(N, generator=g),
           running_var=0.5 + torch.rand(N, generator=g), G=torch.randn(B, N, generator=g))
    i.alpha[0] = 0.0
    i.alpha[-1] = 1.0  # the path through the batch statistics vanishes
    return i


def dice_eval(case, i, dtype):
    z, alpha = _leaf(i.z, dtype), _leaf(i.alpha, dtype)
    y, mean, invstd, var, unbiased = dice(z, None if i.bias is None else i.bias.to(dtype), alpha, BN_EPS)
    dz, dalpha = _grads((y * i.G.to(dtype)).sum(), [z, alpha])
    return dict(y=y.detach(), save_mean=mean.detach(), save_invstd=invstd.detach(), dz=dz, dalpha=dalpha,
                running_mean=BN_MOMENTUM * mean.detach() + (1 - BN_MOMENTUM) * i.running_mean.to(dtype),
                running_var=BN_MOMENTUM * unbiased.detach() + (1 - BN_MOMENTUM) * i.running_var.to(dtype))


PRELU_CASES = [(B, N, per_col, bias) for (B, N), per_col, bias in itertools.product(BN_SHAPES, (False, True),
                                                                                 (True, False))]


def prelu_inputs(case):
    B, N, per_col, bias = case
    g = gen("prelu", case)
    i = NS(z=torch.randn(B, N, generator=g), bias=torch.randn(N, generator=g) if bias else None,
           weight=0.25 + 0.5 * torch.randn(N if per_col else 1, generator=g), G=torch.randn(B, N, generator=g))
    for k in range(min(3, B * N)):  # exact zeros of x
        b, n = (k * 5) % B, (k * 13) % N
        i.z[b, n] = -i.bias[n] if bias else 0.0
    return i


def prelu_eval(case, i, dtype):
    z, w = _leaf(i.z, dtype), _leaf(i.weight, dtype)
    y = prelu(z, None if i.bias is None else i.bias.to(dtype), w)
    dz, dw = _grads((y * i.G.to(dtype)).sum(), [z, w])
    return dict(y=y.detach(), dz=dz, dweight=dw)


# (B, T, H, A2)
DIN_SHAPES = [(1, 1, 8, 4), (5, 7, 6, 5), (6, 65, 16, 40), (9, 130, 32, 40), (3, 20, 64, 8), (7, 9, 48, 12)]
DIN_VOCAB = 23


def din_lens(B, T, g):
    """T, 0, 1, above T, then random lengths."""
    fixed = [T, 0, 1, T + 2]
    return torch.tensor([fixed[b] if b < 4 else int(torch.randint(0, T + 1, (1,), generator=g)) for b in range(B)],
                        dtype=torch.int64)


def din_inputs(shape):
    B, T, H, A2 = shape
    g = gen("din", shape)
    i = NS(q=torch.randn(B, H, generator=g), table=torch.randn(DIN_VOCAB, H, generator=g),
           ids=torch.randint(0, DIN_VOCAB, (B, T), generator=g), z2=torch.randn(B * T, A2, generator=g),
           w3=torch.randn(A2, generator=g) / math.sqrt(A2), b3=torch.randn(1, generator=g),
           dout=torch.randn(B, H, generator=g))
    i.lens = din_lens(B, T, g)
    i.keys = i.table[i.ids]
    i.a2 = torch.relu(i.z2)  # exact zeros, as the att_net's second layer leaves them
    return i


def din_pool_eval(shape, i, dtype, softmax):
    """weights, out, and the gradients of (out * dout).sum() w.r.t. the keys and the pre-relu a2."""
    B, T, H, A2 = shape
    keys, z2 = _leaf(i.keys, dtype), _leaf(i.z2, dtype)
    w, out = din_pool(torch.relu(z2).view(B, T, A2), i.w3.to(dtype), i.b3.to(dtype), keys, i.lens, softmax)
    dkeys, da2 = _grads((out * i.dout.to(dtype)).sum(), [keys, z2])
    return dict(weights=w.detach(), out=out.detach(), dkeys=dkeys, da2=da2)


FOLD_SHAPES = [(B, T, H) for B, T, H, _ in DIN_SHAPES] + [(3, 5, 68), (2, 4, 100)]  # H > 64: din_cross_fold_kernel


def fold_inputs(shape):
    B, T, H = shape
    g = gen("fold", shape)
    return NS(q=torch.randn(B, H, generator=g), keys=torch.randn(B, T, H, generator=g),
              dcross=torch.randn(B * T, 4 * H, generator=g), dkeys0=torch.randn(B, T, H, generator=g),
              dq0=torch.randn(B, H, generator=g))


def fold_eval(shape, i, dtype):
    """The fold accumulates: dkeys0 + d(keys), dq0 + d(query) of (cross * dcross).sum()."""
    B, T, H = shape
    q, k = _leaf(i.q, dtype), _leaf(i.keys, dtype)
    dq, dk = _grads((din_cross(q, k) * i.dcross.to(dtype).view(B, T, 4 * H)).sum(), [q, k])
    return dict(dkeys=i.dkeys0.to(dtype) + dk, dq=i.dq0.to(dtype) + dq)


L2_CASES = list(itertools.product((1, 3, 5), (1, 63, 65, 200)))  # rows, ncols
L2_COL0, L2_LAMBDA, L2_GOUT = 3, 0.2, 0.7


def l2_inputs(case):
    rows, ncols = case
    g = gen("l2", case)
    i = NS(x=torch.randn(rows, L2_COL0 + ncols + 2, generator=g), dx0=torch.randn(rows, L2_COL0 + ncols + 2, generator=g))
    if rows > 1:
        i.x[1, L2_COL0:L2_COL0 + ncols] = 0.0  # a zero-norm row
    return i


def l2_eval(case, i, dtype):
    rows, ncols = case
    v = _leaf(i.x[:, L2_COL0:L2_COL0 + ncols], dtype)
    l2 = row_l2(v, L2_LAMBDA / rows)
    dv, = _grads(l2 * L2_GOUT, [v])
    return dict(l2=l2.detach().reshape(1), dx=i.dx0[:, L2_COL0:L2_COL0 + ncols].to(dtype) + dv)


# (B, F, D, A, nd)
AFM_SHAPES = [(1, 2, 1, 1, 1), (2, 3, 5, 8, 16), (5, 16, 4, 65, 64), (9, 6, 64, 256, 3)]
AFM_VOCAB = 11
AFM_MODES = ("dpred", "dtotal", "both")


def afm_inputs(shape):
    B, Fn, D, A, nd = shape
    P = Fn * (Fn - 1) // 2
    g = gen("afm", shape)
    i = NS(tables=[torch.randn(AFM_VOCAB, D, generator=g) for _ in range(Fn)],
           idx=[torch.randint(0, AFM_VOCAB, (B,), generator=g) for _ in range(Fn)],
           z1=torch.randn(B * P, A, generator=g), w2=torch.randn(A, generator=g) / math.sqrt(A),
           b2=torch.randn(1, generator=g), dense=torch.randn(B, nd, generator=g),
           wd=torch.randn(nd, generator=g) / math.sqrt(nd), bd=torch.randn(1, generator=g),
           wp=torch.randn(D, generator=g) / math.sqrt(D), bp=torch.randn(1, generator=g),
           dpred=torch.randn(B, generator=g), dtotal=torch.randn(B, generator=g),
           d_pairs=torch.randn(B * P, D, generator=g))
    i.emb = torch.stack([t[x] for t, x in zip(i.tables, i.idx)], 1)  # (B, F, D)
    i.pairs = afm_pairs(i.emb)                                          # (B, P, D), exact in fp32
    i.a1 = torch.relu(i.z1)
    return i


def afm_pool_eval(shape, i, dtype, mode):
    B, Fn, D, A, nd = shape
    P = Fn * (Fn - 1) // 2
    z1, pairs = _leaf(i.z1, dtype), _leaf(i.pairs, dtype)
    par = [_leaf(t, dtype) for t in (i.wd, i.bd, i.wp, i.bp, i.w2, i.b2)]
    wd, bd, wp, bp, w2, b2 = par
    delta = torch.zeros(B, P, dtype=dtype, requires_grad=True)  # its gradient is ds, the scores' gradient
    w, ws, logit, pred = afm_pool(torch.relu(z1).view(B, P, A), w2, b2 + delta, pairs, i.dense.to(dtype), wd, bd, wp,
                                  bp)
    loss = 0.0
    if mode in ("dpred", "both"):
        loss = loss + (pred * i.dpred.to(dtype)).sum()
    if mode in ("dtotal", "both"):
        loss = loss + (logit * i.dtotal.to(dtype)).sum()
    g = _grads(loss, [pairs, z1] + par + [delta])
    out = dict(weights=w.detach(), ws=ws.detach(), logit=logit.detach(), pred=pred.detach(),
               d_pairs=g[0].reshape(B * P, D), da1=g[1])
    out.update(zip(("dwd", "dbd", "dwp", "dbp", "dw2", "db2"), g[2:8]))
    # db2 = sum_{b,p} ds_{b,p} is 0 in exact arithmetic (a softmax's Jacobian has zero row sums): its
    # max|want| is the oracle's own rounding noise, so it is compared on the scale of its summands
    out["scale:db2"] = g[8].abs().sum()
    return out


def afm_fold_eval(shape, i, dtype):
    B, Fn, D, A, nd = shape
    e = _leaf(i.emb, dtype)
    de, = _grads((afm_pairs(e).reshape(-1, D) * i.d_pairs.to(dtype)).sum(), [e])
    return dict(d_emb=de.reshape(B, Fn * D))


FM_SHAPES = [(1, 1, 1), (4, 3, 5), (7, 26, 16)]
FM_MODES = ("no_d_deep", "no_dfm2", "both")


def fm_inputs(shape):
    B, Fn, D = shape
    g = gen("fm", shape)
    return NS(e=torch.randn(B, Fn, D, generator=g), d_deep=torch.randn(B, Fn * D, generator=g),
              dfm2=torch.randn(B, generator=g))


def fm_eval(shape, i, dtype, mode):
    B, Fn, D = shape
    e = _leaf(i.e, dtype)
    loss = 0.0
    if mode != "no_d_deep":
        loss = loss + (e.reshape(B, -1) * i.d_deep.to(dtype)).sum()
    if mode != "no_dfm2":
        loss = loss + (fm_second(e) * i.dfm2.to(dtype)).sum()
    de, = _grads(loss, [e])
    return dict(d_e=de.reshape(B, Fn * D))


COMBINE_BATCHES = (1, 255, 257, 600)
COMBINE_GRADS = ("dprob", "dtotal", "dfm1_in", "dfm2_in", "ddeep_in")
COMBINE_CASES = list(itertools.product(COMBINE_BATCHES, (None,) + COMBINE_GRADS))  # (B, the gradient left out)


def combine_inputs(case):
    B, _ = case
    g = gen("combine", B)
    i = NS(fm1=torch.randn(B, generator=g), fm2=torch.randn(B, generator=g), deep=torch.randn(B, generator=g),
           w=torch.randn(3, generator=g), b=torch.randn(1, generator=g))
    for n in COMBINE_GRADS:
        setattr(i, n, torch.randn(B, generator=g))
    return i


def combine_eval(case, i, dtype):
    B, none = case
    leaves = [_leaf(t, dtype) for t in (i.fm1, i.fm2, i.deep, i.w, i.b)]
    fm1, fm2, deep, w, b = leaves
    total, prob = fm_combine(fm1, fm2, deep, w, b)
    loss = 0.0
    for n, t in zip(COMBINE_GRADS, (prob, total, fm1, fm2, deep)):
        if n != none:
            loss = loss + (t * getattr(i, n).to(dtype)).sum()
    g = _grads(loss, leaves)
    return dict(prob=prob.detach(), dfm1=g[0], dfm2=g[1], ddeep=g[2], dfinal_w=g[3], dfinal_b=g[4])


def rel_err(got, want, scale=None):
    """max|got - want| / max|want| (0 / 0 = 0); `scale` replaces max|want| (the eval's "scale:<name>")."""
    scale = float(scale) if scale is not None else float(want.abs().max()) if want.numel() else 0.0
    err = float((got.double() - want.double()).abs().max()) if want.numel() else 0.0
    return (err / scale if scale > 0 else (0.0 if err == 0 else math.inf)), err, scale


def family_evals():
    """family -> list of (case id, eval(dtype) -> dict of compared tensors): every case of the GPU file."""
    fam = {k: [] for k in ("bn_act", "dice", "prelu", "din_pool", "din_fold", "l2", "afm_pool", "afm_fold", "fm")}
    for c in BN_CASES:
        i = bn_inputs(c)
        fam["bn_act"].append((bn_id(c), lambda dt, c=c, i=i: bn_eval(c, i, dt, i.cpu_mask)))
    for c in DICE_CASES:
        i = dice_inputs(c)
        fam["dice"].append((str(c), lambda dt, c=c, i=i: dice_eval(c, i, dt)))
    for c in PRELU_CASES:
        i = prelu_inputs(c)
        fam["prelu"].append((str(c), lambda dt, c=c, i=i: prelu_eval(c, i, dt)))
    for s in DIN_SHAPES:
        i = din_inputs(s)
        for softmax in (False, True):
            fam["din_pool"].append((f"{s} softmax={softmax}",
                                    lambda dt, s=s, i=i, sm=softmax: din_pool_eval(s, i, dt, sm)))
    for s in FOLD_SHAPES:
        i = fold_inputs(s)
        fam["din_fold"].append((str(s), lambda dt, s=s, i=i: fold_eval(s, i, dt)))
    for c in L2_CASES:
        i = l2_inputs(c)
        fam["l2"].append((str(c), lambda dt, c=c, i=i: l2_eval(c, i, dt)))
    for s in AFM_SHAPES:
        i = afm_inputs(s)
        for mode in AFM_MODES:
            fam["afm_pool"].append((f"{s} {mode}", lambda dt, s=s, i=i, m=mode: afm_pool_eval(s, i, dt, m)))
        fam["afm_fold"].append((str(s), lambda dt, s=s, i=i: afm_fold_eval(s, i, dt)))
    for s in FM_SHAPES:
        i = fm_inputs(s)
        for mode in FM_MODES:
            fam["fm"].append((f"{s} {mode}", lambda dt, s=s, i=i, m=mode: fm_eval(s, i, dt, m)))
    for c in COMBINE_CASES:
        i = combine_inputs(c)
        fam["fm"].append((f"combine {c}", lambda dt, c=c, i=i: combine_eval(c, i, dt)))
    return fam
