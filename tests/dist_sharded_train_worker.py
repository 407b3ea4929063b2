"""One rank of tests/test_gpu_sharded_train_pg.py: two ShardedDeepFM.train_step calls (30 fields x
dim 32, hidden [512, 256, 128], B_l 130, dropout 0) over a REAL torch.distributed process group —
gloo with the tensors on cuda:0, since RCCL refuses two ranks on one GPU — with every device step
the real HIP one: all_to_all_single for the index, row and gradient exchanges, all_reduce for the
dense bucket.  Should this gloo build refuse all_reduce on device tensors (probed once with a
one-element tensor on every rank), the rank binds a reduce_fn that stages the bucket through host
memory; the all-to-alls stay on the device either way, and the verdict records which path ran.

Every rank runs the float64 restatement (tests/sharded_train_ref.py) of the global step itself and
compares, after each step, its dense replicas and its own tables under the parameter rule of
test_gpu_sharded_train.py; the restatement is then re-synchronised to the engine (tables and moments
of all owners gathered with all_gather_object).  The verdict, with a checksum of the dense
parameters, goes to RK_OUT as JSON (env: RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT, RK_OUT)."""
import hashlib
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import helpers as H  # noqa: E402,F401  (puts the package on the path)
import sharded_train_ref as S  # noqa: E402
from rankops import sharded  # noqa: E402


def host_reduce(flat):
    host = flat.cpu()
    dist.all_reduce(host, op=dist.ReduceOp.SUM)
    flat.copy_(host)
    return flat


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    res = {"rank": rank, "ok": False}
    try:
        torch.cuda.set_device(0)
        dist.init_process_group("gloo")
        import rankops
        rankops.load_library()
        rows, D, hidden, P, B_l, seed = S.CONFIGS[f"pg30-P{world}"]
        assert P == world
        full = S.initial_model(rows, D, hidden, seed).cuda()
        sh = sharded.ShardedDeepFM.from_deepfm(full, rank=rank, world_size=world).train()
        assert sh.exchange_fn is None and sh.reduce_fn is None  # the real collectives
        try:
            probe = torch.ones(1, device="cuda")
            dist.all_reduce(probe)
            assert float(probe) == world
            res["all_reduce"] = "device"
        except RuntimeError:
            sh.reduce_fn = host_reduce
            res["all_reduce"] = "host-staged"
        tr = S.RefTrainer({k: v.cpu() for k, v in full.state_dict().items()}, rows, hidden, world)
        skip = S.bn_fed_biases(tr.state())
        opts = sh.optimizers(lr=S.LR)
        for step in range(2):
            cats, labels = S.make_batches(rows, world, B_l, seed=seed * 100 + step)
            before = {k: v.detach().cpu().clone() for k, v in sh.state_dict().items()}
            loss = sh.train_step({f: t.cuda() for f, t in cats[rank].items()}, labels[rank].cuda(), opts)
            torch.cuda.synchronize()
            _, want_losses = tr.forward_backward(cats, labels)
            tr.step(cats)
            torch.testing.assert_close(loss.cpu(), want_losses[rank].detach().float(), rtol=1e-4, atol=1e-4)
            touched = tr.batch_rows(cats)
            for k, p in sh.named_parameters():
                got, want = p.detach().cpu(), tr.p[k].detach()
                if k in touched:
                    mask = torch.zeros(got.shape[0], dtype=torch.bool)
                    mask[touched[k]] = True
                    assert torch.equal(got[~mask], before[k][~mask]), f"{k}: rows outside the global batch moved"
                    got, want = got[mask], want[mask]
                if k not in skip:
                    S.adam_rule(got, want, S.LR, f"step {step} param {k}")
            for k, v in sh.state_dict().items():
                if k in tr.buf:
                    torch.testing.assert_close(v.cpu(), tr.buf[k].to(v.dtype), rtol=1e-4, atol=1e-4,
                                               msg=lambda m: f"step {step} buffer {k}: {m}")
            # re-synchronise the restatement to the engine: this rank's view, then every owner's tables
            mine = {k: v.detach().cpu() for k, v in sh.state_dict().items()}
            mom = {k: (opts[1 if S.is_table(k) else 0].state[p]["exp_avg"].cpu(),
                       opts[1 if S.is_table(k) else 0].state[p]["exp_avg_sq"].cpu())
                   for k, p in sh.named_parameters()}
            gathered = [None] * world
            dist.all_gather_object(gathered, ({k: v for k, v in mine.items() if S.is_table(k)},
                                              {k: v for k, v in mom.items() if S.is_table(k)}))
            state = {k: v for k, v in mine.items() if not S.is_table(k)}
            tmom = {}
            for tabs, moms in gathered:
                state.update(tabs)
                tmom.update(moms)
            tr.load(state, {k: v for k, v in mom.items() if not S.is_table(k)}, tmom)
        dense = torch.cat([p.detach().reshape(-1) for k, p in sh.named_parameters() if not S.is_table(k)]
                          + [b.detach().float().reshape(-1) for b in sh.buffers()])
        res["dense_checksum"] = hashlib.sha256(dense.cpu().numpy().tobytes()).hexdigest()
        res["error_flags"] = int(rankops.error_flags())
        assert res["error_flags"] == 0
        res["ok"] = True
    except Exception as exc:  # reported to the parent test
        res["error"] = traceback.format_exc()[-3000:] + repr(exc)
    finally:
        with open(os.environ["RK_OUT"], "w") as f:
            json.dump(res, f)
        if dist.is_initialized():
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
