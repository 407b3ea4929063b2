"""Op-level GPU tests of ShardedDeepFM's three training kernels (csrc/shard_train.hip): each
rankops.ops wrapper is called directly into sentinel-guarded buffers (the Guard / Flat pattern of
test_gpu_train_ops.py) at the smallest shapes that can go wrong: B_l 1 and 3 (the pad4 tail), 5, 67
(past a 64-sample workgroup at D = 4), D 4 .. 64 (16 .. 1 samples' lane groups per wave), and field /
owner counts with uneven owners ((30, 8): 4/4/4/4/4/4/3/3) and an owner without fields ((3, 4)).

rk_shard_unpack_grads and rk_shard_fm_assemble move data: bit-equal to torch indexing of the same
buffers (tests/sharded_train_ref.py), ids int64 with -1 preserved; assemble's fm1 is the owners'
partials added in owner order (bit-equal to the same float32 adds), its fm2 is arithmetic and is held
to the float64 restatement by the close rule with REL["fm"] (max|want|), except where max|want|
degenerates: at one field fm2 is exactly zero (the two sums cancel) and at one sample it is a single
value that may cancel, while a float32 evaluation keeps the rounding of each square; there the scale
is that of the summands, 0.5 (sum_d S_d^2 + sum_{f,d} e^2), as test_gpu_train_ops.py treats AFM's db2.  rk_shard_fm_backward_pack is held to the float64
train_ops_ref.fm_eval gradient rearranged into the wire layout and multiplied by scale, by the close
rule and REL["fm"] of test_gpu_train_ops.py (the project's bound for this arithmetic); its first-order
tails are bit-equal to dfm1 * float32(scale) and the pad lanes exactly zero."""
from types import SimpleNamespace as NS

import pytest
import torch

import rankops
import sharded_train_ref as S
import train_ops_ref as R
from rankops import ops
from test_gpu_train_ops import REL, SENT, Flat, Guard, close, invalid

pytestmark = pytest.mark.gpu

f64 = torch.float64
BATCHES = (1, 3, 5, 67)
DIMS = (4, 8, 32, 64)
LAYOUTS = ((1, 1), (7, 2), (7, 3), (30, 8), (3, 4))  # (fields, owners)
MODES = ("no_d_deep", "no_dfm2", "both")
SCALES = (1.0, 0.5, 1.0 / 3.0)
RK_FLAG_INDEX_OOB = 1  # include/rankops.h


def gen(*key):
    return R.gen("shard_train", *key)


def wire_floats(B, Fn, P, D):
    return sum(S.block(B, len(fr), D) for fr in S.fields_of(Fn, P))


class Bytes:
    """Typed tensors carved at 16-B aligned offsets from one 0x5A-filled byte buffer with 64 guard
    bytes around each; check() asserts that every byte outside the carved tensors is untouched."""

    def __init__(self):
        self.specs, self.n = [], 64

    def add(self, dtype, *shape):
        n = torch.empty((), dtype=dtype).element_size()
        for s in shape:
            n *= s
        self.specs.append((self.n, n, dtype, shape))
        self.n += (n + 15) // 16 * 16 + 64
        return len(self.specs) - 1

    def build(self):
        self.buf = torch.full((self.n,), 0x5A, dtype=torch.uint8, device="cuda")
        return [self.buf[o:o + n].view(dt).view(*shape) for o, n, dt, shape in self.specs]

    def check(self, what):
        rest = self.buf.clone()
        for o, n, _, _ in self.specs:
            rest[o:o + n] = 0x5A
        assert bool((rest == 0x5A).all()), f"{what}: stored outside its range"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_fm_assemble_is_the_indexing_and_the_fm_sums(layout, B):
    Fn, P = layout
    for D in DIMS:
        recv = torch.randn(wire_floats(B, Fn, P, D), generator=gen("asm", layout, B, D))
        deep_in, fm1, fm2 = Guard(B, Fn * D, c0=4, pad=4), Flat(B, 1), Flat(B, 1)
        ops.shard_fm_assemble(recv.cuda(), Fn, P, D, deep_in.v, fm1.v, fm2.v)
        want_in, want_fm1, _ = S.assemble(recv, Fn, P, D, B)
        assert torch.equal(deep_in.check("deep_in").cpu(), want_in), (layout, B, D)
        assert torch.equal(fm1.check("fm1").view(B).cpu(), want_fm1), (layout, B, D)
        scale = None  # the close rule: max|want|
        if Fn == 1 or B == 1:
            e = S.assemble(recv.double(), Fn, P, D, B)[0].view(B, Fn, D)
            scale = float((0.5 * (e.sum(1) ** 2 + (e * e).sum(1)).sum(1)).max())
        close("fm2", fm2.check("fm2").view(B), S.assemble(recv.double(), Fn, P, D, B)[2], REL["fm"], scale=scale)
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_unpack_grads_is_the_indexing(layout, B):
    Fn, P = layout
    for D in DIMS:
        for F_me in sorted({len(fr) for fr in S.fields_of(Fn, P)}):
            g = gen("unpack", layout, B, D, F_me)
            recv = torch.randn(P * S.block(B, F_me, D), generator=g)
            idx = torch.randint(0, 1000, (P * B * max(F_me, 1),), generator=g, dtype=torch.int32)[:P * B * F_me]
            if idx.numel():
                idx[int(torch.randint(0, idx.numel(), (1,), generator=g))] = -1
            N = P * B
            mem = Bytes()
            for dt, shape in ((torch.int64, (max(F_me, 1), N)), (torch.float32, (max(F_me, 1), N, D)),
                              (torch.float32, (N,))):
                mem.add(dt, *shape)
            ids, v2, v1 = mem.build()
            before = mem.buf.clone()
            ops.shard_unpack_grads(recv.cuda(), idx.cuda(), F_me, D, P, B, ids, v2, v1)
            mem.check("unpack")
            if F_me == 0:  # an owner without fields: RK_OK, no launch, nothing written
                assert torch.equal(mem.buf, before)
                continue
            w_ids, w_v2, w_v1 = S.unpack(recv, idx, F_me, D, P, B)
            assert ids.dtype == torch.int64 and torch.equal(ids.cpu(), w_ids), (layout, B, D)
            assert int((ids == -1).sum()) == 1
            assert torch.equal(v2.cpu(), w_v2) and torch.equal(v1.cpu(), w_v1), (layout, B, D)
    assert rankops.error_flags() == 0


def run_pack(layout, B, D, mode, scale):
    Fn, P = layout
    g = gen("pack", layout, B, D)
    i = NS(e=torch.randn(B, Fn, D, generator=g), d_deep=torch.randn(B, Fn * D, generator=g),
           dfm2=torch.randn(B, generator=g))
    dfm1 = torch.randn(B, generator=g)
    deep_in = Guard(B, Fn * D, c0=4, pad=4, fill=i.e.reshape(B, Fn * D))
    d_deep = Guard(B, Fn * D, c0=8, pad=0, fill=i.d_deep) if mode != "no_d_deep" else None
    dfm2 = i.dfm2.cuda().view(B, 1) if mode != "no_dfm2" else None
    out = Flat(wire_floats(B, Fn, P, D))
    ops.shard_fm_backward_pack(deep_in.v, None if d_deep is None else d_deep.v, dfm2, dfm1.cuda().view(B, 1), scale,
                               Fn, P, D, out.v)
    s32 = torch.tensor(scale, dtype=torch.float32)
    want = S.backward_pack(R.fm_eval((B, Fn, D), i, f64, mode)["d_e"], dfm1.double(), float(s32), Fn, P, D, B)
    got = out.check("send buffer")
    deep_in.check("deep_in")
    gb, wb = S.owner_blocks(got.cpu(), Fn, P, D, B), S.owner_blocks(want, Fn, P, D, B)
    rows = [(a[0].reshape(-1), b[0].reshape(-1)) for a, b in zip(gb, wb) if a is not None]
    close(f"rows {layout} B={B} D={D} {mode} scale={scale:.3f}", torch.cat([a for a, _ in rows]),
          torch.cat([b for _, b in rows]), REL["fm"])
    for blk in gb:
        if blk is not None:
            assert torch.equal(blk[1][:B], dfm1 * s32), "first-order tail"
            assert bool((blk[1][B:] == 0).all()), "pad lanes"


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_fm_backward_pack(layout, B):
    """Every shape; the three modes and the three scales rotate over the shapes (each pair occurs)."""
    k = LAYOUTS.index(layout) * len(BATCHES) + BATCHES.index(B)
    for d, D in enumerate(DIMS):
        n = k * len(DIMS) + d
        run_pack(layout, B, D, MODES[n % 3], SCALES[(n // 3) % 3])
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("scale", SCALES, ids=lambda s: f"{s:.3f}")
@pytest.mark.parametrize("mode", MODES)
def test_fm_backward_pack_modes_and_scales(mode, scale):
    run_pack((7, 3), 5, 8, mode, scale)
    run_pack((30, 8), 67, 32, mode, scale)
    assert rankops.error_flags() == 0


def test_refused_calls_write_nothing():
    B, Fn, P, D = 5, 7, 3, 8

    def buffers(Fn=Fn, P=P, D=D, offset=0):
        # the leading dimension stays a multiple of 4 floats whatever D is (D = 6: 42 columns in rows of
        # 52), and every buffer 16-B aligned unless `offset` says otherwise: a refusal is then for the
        # condition the case names alone
        b = NS(recv=torch.zeros(wire_floats(B, Fn, P, D) + 4 + 1, device="cuda")[offset:],
               deep_in=Guard(B, Fn * D, c0=4 + offset, pad=4 - offset + -(Fn * D) % 4), fm1=Flat(B, 1), fm2=Flat(B, 1),
               out=Flat(wire_floats(B, Fn, P, D) + -wire_floats(B, Fn, P, D) % 4, offset=offset),
               dfm1=torch.zeros(B, 1, device="cuda"))
        assert b.deep_in.v.stride(0) % 4 == 0 and b.deep_in.v.stride(0) >= Fn * D
        for t in (b.recv, b.deep_in.v, b.out.v):
            assert t.data_ptr() % 16 == 4 * offset
        return b

    def untouched(b):
        for t in (b.deep_in, b.fm1, b.fm2, b.out):
            t.check("refused call")
            assert bool((t.v == SENT).all())

    for kw in (dict(D=6), dict(Fn=33, P=1)):  # dim % 4, more than 32 fields on one owner
        b = buffers(**kw)
        Fk, Pk, Dk = kw.get("Fn", Fn), kw.get("P", P), kw.get("D", D)
        invalid(ops.shard_fm_assemble, b.recv, Fk, Pk, Dk, b.deep_in.v, b.fm1.v, b.fm2.v)
        invalid(ops.shard_fm_backward_pack, b.deep_in.v, None, None, b.dfm1, 1.0, Fk, Pk, Dk, b.out.v)
        untouched(b)
    b = buffers()  # NULL outputs
    invalid(ops.shard_fm_assemble, b.recv, Fn, P, D, b.deep_in.v, None, b.fm2.v)
    invalid(ops.shard_fm_assemble, b.recv, Fn, P, D, b.deep_in.v, b.fm1.v, None)
    invalid(ops.shard_fm_backward_pack, b.deep_in.v, None, None, b.dfm1, 1.0, Fn, P, D, None)
    invalid(ops.shard_fm_backward_pack, b.deep_in.v, None, None, None, 1.0, Fn, P, D, b.out.v)
    untouched(b)
    b = buffers(offset=1)  # one float off 16-B alignment: the input, then each output
    a = buffers()
    invalid(ops.shard_fm_assemble, b.recv, Fn, P, D, a.deep_in.v, a.fm1.v, a.fm2.v)
    invalid(ops.shard_fm_assemble, a.recv, Fn, P, D, b.deep_in.v, a.fm1.v, a.fm2.v)
    invalid(ops.shard_fm_backward_pack, b.deep_in.v, None, None, a.dfm1, 1.0, Fn, P, D, a.out.v)
    invalid(ops.shard_fm_backward_pack, a.deep_in.v, None, None, a.dfm1, 1.0, Fn, P, D, b.out.v)
    untouched(a)
    untouched(b)

    F_me, N = 3, P * B
    recv = torch.zeros(P * S.block(B, F_me, D) + 1, device="cuda")
    idx = torch.zeros(N * 33, dtype=torch.int32, device="cuda")
    mem = Bytes()
    for dt, shape in ((torch.int64, (33, N)), (torch.float32, (33, N, D + 1)), (torch.float32, (N,))):
        mem.add(dt, *shape)
    ids, v2, v1 = mem.build()
    before = mem.buf.clone()
    invalid(ops.shard_unpack_grads, recv, idx, F_me, 6, P, B, ids, v2, v1)
    invalid(ops.shard_unpack_grads, recv, idx, 33, D, P, B, ids, v2, v1)
    invalid(ops.shard_unpack_grads, recv, idx, F_me, D, P, B, None, v2, v1)
    invalid(ops.shard_unpack_grads, recv, idx, F_me, D, P, B, ids, None, v1)
    invalid(ops.shard_unpack_grads, recv, idx, F_me, D, P, B, ids, v2, None)
    invalid(ops.shard_unpack_grads, recv[1:], idx, F_me, D, P, B, ids, v2, v1)
    invalid(ops.shard_unpack_grads, recv, idx, F_me, D, P, B, ids, v2.view(-1)[1:], v1)
    assert torch.equal(mem.buf, before)
    assert rankops.error_flags() == 0


def test_a_minus_one_id_is_dropped_and_flagged_at_the_optimizer_step():
    """An id the index exchange sent as -1 stays -1 through the unpack; rk_sparse_adam_step drops the
    entry and raises RK_FLAG_INDEX_OOB: table 0 (all ids -1) does not move at all, table 1 moves
    exactly the rows of its ids."""
    P, B, D, F_me, V = 2, 3, 8, 2, 11
    g = gen("minus_one")
    N = P * B
    recv = torch.randn(P * S.block(B, F_me, D), generator=g) + 3.0
    idx = torch.randint(0, V, (P, B, F_me), generator=g, dtype=torch.int32)
    idx[:, :, 0] = -1
    ids = torch.empty(F_me, N, dtype=torch.int64, device="cuda")
    v2 = torch.empty(F_me, N, D, device="cuda")
    v1 = torch.empty(N, device="cuda")
    ops.shard_unpack_grads(recv.cuda(), idx.cuda().view(-1), F_me, D, P, B, ids, v2, v1)
    assert bool((ids[0] == -1).all()) and torch.equal(ids[1].cpu(), idx[:, :, 1].reshape(-1).long())
    assert rankops.error_flags() == 0
    tables = [torch.nn.Parameter(torch.randn(V, D, generator=g).cuda()) for _ in range(F_me)]
    start = [t.detach().clone() for t in tables]
    for j, t in enumerate(tables):
        t.grad = torch.sparse_coo_tensor(ids[j].unsqueeze(0), v2[j], t.shape, check_invariants=False)
    rankops.SparseAdam(tables, lr=1e-2).step()
    assert rankops.error_flags() == RK_FLAG_INDEX_OOB
    assert torch.equal(tables[0].detach(), start[0])
    moved = (tables[1].detach() != start[1]).any(1).cpu()
    want = torch.zeros(V, dtype=torch.bool)
    want[idx[:, :, 1].reshape(-1).long()] = True
    assert torch.equal(moved, want)
