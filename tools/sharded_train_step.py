"""ShardedDeepFM's training step against DeepFM(sparse_grad=True), and its three kernels alone.

Tables of DeepFM configs[1]'s size (30 fields x 1,000,000 rows x 32), graph-free eager steps, timed
with device events after warm-up (an eager step of ~60 launches is partly host-bound: the host
clock per step is printed beside the event time):

  step      B 4096: the P = 1 sharded step (train_step: index pack + copy, split gather + copy,
            assemble, tail, backward, backward-pack, copy, unpack, both optimizers) and the
            DeepFM(sparse_grad=True) step (rankops.Adam + rankops.SparseAdam) on equal weights
  pieces    B 4096, P = 1: what the sharded step adds to the single-GPU one, launch by launch
            (index pack, split gather, assemble, backward-pack, unpack, and a copy of each of the
            three exchanged buffers) and what it replaces (rk_fm_gather, rk_fm_backward +
            rk_pack_blocks)
  kernels   P = 8 emulated, B_l 8192 (configs[4]'s local batch): rk_shard_fm_assemble (30 fields),
            rk_shard_fm_backward_pack (30 fields), rk_shard_unpack_grads (rank 0: 4 fields x 8
            sources), each alone over random buffers, with the bytes it moves

Needs a GPU; prints one JSON line per leg."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402,F401  (sets sys.path for rankops and tests/)
import torch  # noqa: E402

import rankops  # noqa: E402
from rankops import ops, train  # noqa: E402
from rankops.sharded import ShardedDeepFM  # noqa: E402

FIELDS = {f"field_{i:02d}": 1_000_000 for i in range(30)}
DIM = 32


def timed(fn, steps, warmup):
    """(event ms per call, host ms per call) over `steps` calls after `warmup`."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / steps, 4), round(1e3 * (time.perf_counter() - t0) / steps, 4)


def step_legs(batch, steps, warmup):
    torch.manual_seed(0)
    with torch.device("cuda"):
        full = rankops.DeepFM(None, embedding_dim=DIM, vocab_sizes={f: n - 1 for f, n in FIELDS.items()},
                              sparse_grad=True)
    full = full.cuda().train()
    sh = ShardedDeepFM.from_deepfm(full).train()
    g = torch.Generator().manual_seed(77)
    cat = {f: torch.randint(0, n, (batch,), generator=g).cuda() for f, n in FIELDS.items()}
    label = (torch.rand(batch, generator=g) < 0.3).float().cuda()
    tables = [p for m in full.modules() if isinstance(m, torch.nn.Embedding) for p in m.parameters()]
    ids = {id(p) for p in tables}
    opts = [rankops.Adam([p for p in full.parameters() if id(p) not in ids], lr=1e-3),
            rankops.SparseAdam(tables, lr=1e-3)]
    crit = torch.nn.BCELoss()

    def single():
        for o in opts:
            o.zero_grad(set_to_none=True)
        crit(full(cat)[0].squeeze(), label).backward()
        for o in opts:
            o.step()

    sh_opts = sh.optimizers(lr=1e-3)
    ev, host = timed(single, steps, warmup)
    print(json.dumps({"leg": "step", "model": "DeepFM(sparse_grad=True)", "batch": batch, "event_ms": ev,
                      "host_ms": host}), flush=True)
    ev, host = timed(lambda: sh.train_step(cat, label, sh_opts), steps, warmup)
    print(json.dumps({"leg": "step", "model": "ShardedDeepFM P=1", "batch": batch, "event_ms": ev, "host_ms": host}),
          flush=True)
    pieces(sh, full, cat, batch, steps, warmup)
    assert rankops.error_flags() == 0


def pieces(sh, full, cat, B, steps, warmup):
    F, D = len(FIELDS), DIM
    dev = "cuda"
    recv_idx = sh.exchange_indices(cat, B)
    rows = sh._gather_split(recv_idx, B, 0, B)
    deep_in, d_deep = torch.empty(B, F * D, device=dev), torch.randn(B, F * D, device=dev)
    fm1, fm2, dfm1, dfm2 = (torch.randn(B, 1, device=dev) for _ in range(4))
    send = torch.empty_like(rows)
    N = B
    ids = torch.empty(F, N, dtype=torch.int64, device=dev)
    v2, v1 = torch.empty(F, N, D, device=dev), torch.empty(N, device=dev)
    names = list(FIELDS)
    idx = [cat[f] for f in names]
    second = ops.table_seg_array([full.second_order_embeddings[n].weight for n in names], idx,
                                 [f * D for f in range(F)])
    first = ops.table_seg_array([full.first_order_embeddings[n].weight for n in names], idx, list(range(F)))
    d_second = torch.empty(B, F * D, device=dev)
    w = [full.first_order_embeddings[n].weight for n in names] + [full.second_order_embeddings[n].weight for n in names]
    src = [[(i, dfm1, 0)] for i in idx] + [[(i, d_second, f * D)] for f, i in enumerate(idx)]
    legs = {
        "index pack (rk_shard_pack_indices)": lambda: sh.pack_indices(cat),
        "split gather (rk_shard_gather_rows_split)": lambda: sh._gather_split(recv_idx, B, 0, B),
        "assemble (rk_shard_fm_assemble)": lambda: ops.shard_fm_assemble(rows, F, 1, D, deep_in, fm1, fm2),
        "backward-pack (rk_shard_fm_backward_pack)":
            lambda: ops.shard_fm_backward_pack(deep_in, d_deep, dfm2, dfm1, 1.0, F, 1, D, send),
        "unpack (rk_shard_unpack_grads)": lambda: ops.shard_unpack_grads(send, recv_idx, F, D, 1, B, ids, v2, v1),
        "copy of the index buffer": lambda: torch.empty_like(recv_idx).copy_(recv_idx),
        "copy of the row buffer": lambda: torch.empty_like(rows).copy_(rows),
        "copy of the gradient buffer": lambda: torch.empty_like(send).copy_(send),
        "replaced: rk_fm_gather": lambda: ops.fm_gather(second, first, D, B, deep_in, fm1, fm2),
        "replaced: rk_fm_backward": lambda: ops.fm_backward(deep_in, d_deep, dfm2, F, D, d_second),
        "replaced: sparse_embedding_grads (rk_pack_blocks)": lambda: train.sparse_embedding_grads(w, src),
    }
    for name, fn in legs.items():
        ev, host = timed(fn, steps, warmup)
        print(json.dumps({"leg": "pieces", "what": name, "batch": B, "event_us": round(1e3 * ev, 2),
                          "host_us": round(1e3 * host, 2)}), flush=True)


def kernel_legs(B, steps, warmup):
    F, P, D, dev = 30, 8, DIM, "cuda"
    F_me = 4
    wire = sum(B * (F // P + (r < F % P)) * D + (B + 3) // 4 * 4 for r in range(P))
    recv = torch.randn(wire, device=dev)
    deep_in, d_deep = torch.empty(B, F * D, device=dev), torch.randn(B, F * D, device=dev)
    fm1, fm2, dfm1, dfm2 = (torch.randn(B, 1, device=dev) for _ in range(4))
    send = torch.empty(wire, device=dev)
    grecv = torch.randn(P * (B * F_me * D + (B + 3) // 4 * 4), device=dev)
    idx = torch.randint(0, 1_000_000, (P * B * F_me,), dtype=torch.int32, device=dev)
    N = P * B
    ids = torch.empty(F_me, N, dtype=torch.int64, device=dev)
    v2, v1 = torch.empty(F_me, N, D, device=dev), torch.empty(N, device=dev)
    legs = [
        ("rk_shard_fm_assemble", lambda: ops.shard_fm_assemble(recv, F, P, D, deep_in, fm1, fm2),
         4 * (wire + B * F * D + 2 * B)),
        ("rk_shard_fm_backward_pack", lambda: ops.shard_fm_backward_pack(deep_in, d_deep, dfm2, dfm1, 1 / P, F, P, D, send),
         4 * (2 * B * F * D + 2 * B + wire)),
        ("rk_shard_unpack_grads", lambda: ops.shard_unpack_grads(grecv, idx, F_me, D, P, B, ids, v2, v1),
         4 * grecv.numel() + 4 * idx.numel() + 8 * ids.numel() + 4 * v2.numel() + 4 * v1.numel()),
    ]
    for name, fn, nbytes in legs:
        ev, _ = timed(fn, steps, warmup)
        print(json.dumps({"leg": "kernels", "kernel": name, "P": P, "B_l": B, "event_us": round(1e3 * ev, 2),
                          "bytes": nbytes, "GB_per_s": round(nbytes / (ev * 1e-3) / 1e9, 1)}), flush=True)
    assert rankops.error_flags() == 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--local-batch", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sharded_train_step.py needs a ROCm GPU")
    kernel_legs(args.local_batch, 4 * args.steps, args.warmup)
    step_legs(args.batch, args.steps, args.warmup)


if __name__ == "__main__":
    main()
