"""GPU tests of ShardedDeepFM's hybrid-parallel training step (rankops/sharded.py).

The P ranks are threads of this process on one device: the all-to-alls go through
a2a_emulator.InProcessAllToAll, the dense reduction through allreduce_emulator.InProcessAllReduce;
every device step of every rank is the real one.  The oracle is tests/sharded_train_ref.py (float64;
tied to autograd by test_sharded_train_ref.py).

Bounds (none of them new): outputs and BatchNorm buffers assert_close(rtol 1e-4, atol 1e-4); every
gradient atol = 2e-4 * max(1e-3, max|want|) (test_gpu_train.py / test_gpu_sparse_train.py); parameters
after a step by _assert_adam_params_close of test_gpu_train.py (sharded_train_ref.adam_rule), a Linear
bias that feeds a BatchNorm left out as _deepfm_step_check leaves it out (zero true gradient); table
rows outside the global batch bit-unchanged."""
import pytest
import torch

import helpers as H
import rankops
import sharded_train_ref as S
import sparse_models as M
from a2a_emulator import InProcessAllToAll, run_ranks
from allreduce_emulator import InProcessAllReduce
from oracle import reference_forward as ref
from rankops.sharded import ShardedDeepFM

pytestmark = pytest.mark.gpu


def grad_close(got, want, what):
    want = want.float()
    atol = 2e-4 * max(1e-3, float(want.abs().max()) if want.numel() else 0.0)
    torch.testing.assert_close(got.cpu(), want, rtol=0, atol=atol, msg=lambda m: f"{what}: {m}")


class Ranks:
    """P shards of one full DeepFM with the emulated collectives bound, and their optimizers."""

    def __init__(self, full, P):
        self.P = P
        self.a2a, self.ar = InProcessAllToAll(P), InProcessAllReduce(P)
        self.shards = []
        for r in range(P):
            sh = ShardedDeepFM.from_deepfm(full, rank=r, world_size=P).train()
            sh.exchange_fn, sh.reduce_fn = self.a2a.bind(r), self.ar.bind(r)
            self.shards.append(sh)
        self.opts = [sh.optimizers(lr=S.LR) for sh in self.shards]

    def run(self, fn):
        def abort():
            self.a2a.abort()
            self.ar.abort()
        out = run_ranks(self.P, lambda r: fn(r, self.shards[r]), on_error=abort)
        torch.cuda.synchronize()
        return out

    def backward(self, cats, labels):
        """zero_grad, forward, local BCE, backward, sync_gradients on every rank; the outputs."""
        def body(r, sh):
            for o in self.opts[r]:
                if o is not None:
                    o.zero_grad()
            out = sh({f: t.cuda() for f, t in cats[r].items()})
            torch.nn.functional.binary_cross_entropy(out[0].reshape(-1), labels[r].cuda()).backward()
            sh.sync_gradients()
            return [o.detach() for o in out]
        return self.run(body)

    def step(self):
        def body(r, sh):
            for o in self.opts[r]:
                if o is not None:
                    o.step()
        self.run(body)

    def train_steps(self, batches):
        def body(r, sh):
            return [sh.train_step({f: t.cuda() for f, t in cats[r].items()}, labels[r].cuda(), self.opts[r])
                    for cats, labels in batches]
        return self.run(body)

    def state(self):
        """The gathered full state_dict (dense entries from rank 0, every table from its owner), on the CPU."""
        out = {}
        for r, sh in enumerate(self.shards):
            for k, v in sh.state_dict().items():
                if S.is_table(k) or r == 0:
                    out[k] = v.detach().cpu().clone()
        return out

    def moments(self):
        dense, tables = {}, {}
        for k, p in self.shards[0].named_parameters():
            if not S.is_table(k):
                st = self.opts[0][0].state[p]
                dense[k] = (st["exp_avg"].cpu(), st["exp_avg_sq"].cpu())
        for r, sh in enumerate(self.shards):
            for k, p in sh.named_parameters():
                if S.is_table(k):
                    st = self.opts[r][1].state[p]
                    tables[k] = (st["exp_avg"].cpu(), st["exp_avg_sq"].cpu())
        return dense, tables


# ------------------------------------------------------------------ 1. P = 1 is the single-GPU model

def hyperparameters(model):
    return [(type(l).__name__, l.p) if isinstance(l, torch.nn.Dropout) else (type(l).__name__, l.eps, l.momentum)
            for l in model.deep_layers if isinstance(l, (torch.nn.Dropout, torch.nn.BatchNorm1d))]


def test_one_rank_equals_deepfm_with_sparse_gradients():
    one_rank_check(M.build("deepfm", True).cuda().train())  # dropout 0.1, BatchNorm defaults


def test_from_deepfm_carries_dropout_and_batchnorm_hyperparameters():
    """What the state_dict does not carry: a dropout rate of 0.5 and BatchNorm eps / momentum away
    from the defaults reach the shard, and the P = 1 step equals the single-GPU model with them."""
    full = M.build("deepfm", True)
    for l in full.deep_layers:
        if isinstance(l, torch.nn.Dropout):
            l.p = 0.5
        elif isinstance(l, torch.nn.BatchNorm1d):
            l.eps, l.momentum = 1e-3, 0.3
    full = full.cuda().train()
    sh = one_rank_check(full)
    assert ("Dropout", 0.5) in hyperparameters(sh) and ("BatchNorm1d", 1e-3, 0.3) in hyperparameters(sh)
    plain = ShardedDeepFM.from_deepfm(M.build("deepfm", True).cuda())
    assert ("Dropout", 0.1) in hyperparameters(plain) and ("BatchNorm1d", 1e-5, 0.1) in hyperparameters(plain)


def one_rank_check(full):
    sh = ShardedDeepFM.from_deepfm(full).train()
    assert hyperparameters(sh) == hyperparameters(full) and len(hyperparameters(sh)) == 4
    inp = H.to_device(M.inputs("deepfm"), "cuda")
    label = M.labels().cuda()
    outs = []
    for m in (full, sh):
        torch.manual_seed(1234)  # the dropout streams take torch.initial_seed() at their first use
        out = m(inp["category"])
        torch.nn.functional.binary_cross_entropy(out[0].reshape(-1), label).backward()
        outs.append(out)
    sh.sync_gradients()
    for i, (a, b) in enumerate(zip(outs[1], outs[0])):
        torch.testing.assert_close(a.detach(), b.detach(), rtol=1e-4, atol=1e-4, msg=lambda m: f"output {i}: {m}")
    want = dict(full.named_parameters())
    n_tables = 0
    for k, p in sh.named_parameters():
        g, w = p.grad, want[k].grad
        if S.is_table(k):
            n_tables += 1
            assert g.is_sparse and not g.is_coalesced() and g._nnz() == M.B, k
            g, w = g.to_dense(), w.to_dense()
        grad_close(g, w.cpu(), k)
    assert n_tables == 12
    for k, v in sh.state_dict().items():
        if k not in want:
            torch.testing.assert_close(v, full.state_dict()[k], rtol=1e-4, atol=1e-4, msg=lambda m: f"{k}: {m}")
    assert rankops.error_flags() == 0
    return sh


# ------------------------------------------------------------------ 2. P ranks against the restatement

@pytest.mark.parametrize("name", list(S.CONFIGS))
def test_steps_match_the_float64_restatement(name):
    rows, D, hidden, P, B, seed = S.CONFIGS[name]
    full = S.initial_model(rows, D, hidden, seed).cuda()
    ranks = Ranks(full, P)
    tr = S.RefTrainer(ranks.state(), rows, hidden, P)
    skip = S.bn_fed_biases(tr.state())
    for step in range(3):
        cats, labels = S.make_batches(rows, P, B, seed=seed * 100 + step)
        outs = ranks.backward(cats, labels)
        want_outs, _ = tr.forward_backward(cats, labels)
        before = ranks.state()
        for r, sh in enumerate(ranks.shards):
            for i, (a, b) in enumerate(zip(outs[r], want_outs[r])):
                torch.testing.assert_close(a.cpu(), b.detach().float(), rtol=1e-4, atol=1e-4,
                                           msg=lambda m: f"step {step} rank {r} output {i}: {m}")
            for k, v in sh.state_dict().items():
                if k in tr.buf:
                    torch.testing.assert_close(v.cpu(), tr.buf[k].to(v.dtype), rtol=1e-4, atol=1e-4,
                                               msg=lambda m: f"step {step} rank {r} buffer {k}: {m}")
            for k, p in sh.named_parameters():
                g = p.grad
                if S.is_table(k):
                    assert g.is_sparse and g._nnz() == P * B, k
                    g = g.to_dense()
                grad_close(g, tr.p[k].grad, f"step {step} rank {r} grad {k}")
        ranks.step()
        tr.step(cats)
        touched = tr.batch_rows(cats)
        for r, sh in enumerate(ranks.shards):
            for k, p in sh.named_parameters():
                got, want = p.detach().cpu(), tr.p[k].detach()
                if k in touched:
                    mask = torch.zeros(got.shape[0], dtype=torch.bool)
                    mask[touched[k]] = True
                    assert torch.equal(got[~mask], before[k][~mask]), f"{k}: rows outside the global batch moved"
                    got, want = got[mask], want[mask]
                if k not in skip:
                    S.adam_rule(got, want, S.LR, f"step {step} rank {r} param {k}")
        tr.load(ranks.state(), *ranks.moments())  # every step is checked from the engine's state
    assert rankops.error_flags() == 0


# ------------------------------------------------------------------ 3. replicas stay identical

def three_steps(seed=21):
    rows, D, hidden, P, B = S.WECHAT7, 8, [32, 16], 3, 33
    ranks = Ranks(S.initial_model(rows, D, hidden, seed, dropout=0.1).cuda(), P)
    torch.manual_seed(seed)
    losses = ranks.train_steps([S.make_batches(rows, P, B, seed=seed * 100 + i) for i in range(3)])
    return ranks, losses


def test_replicas_are_bit_identical_and_runs_repeat():
    ranks, losses = three_steps()
    assert all(torch.isfinite(l).all() for ls in losses for l in ls)
    first, opt0 = ranks.shards[0], ranks.opts[0][0]
    names = [k for k, _ in first.named_parameters() if not S.is_table(k)]
    assert len(names) >= 10
    for r in range(1, ranks.P):
        sh = ranks.shards[r]
        params = dict(sh.named_parameters())
        for k, p in first.named_parameters():
            if S.is_table(k):
                continue
            assert torch.equal(p, params[k]), f"rank {r} {k}"
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(opt0.state[p][key], ranks.opts[r][0].state[params[k]][key]), f"rank {r} {k} {key}"
        sd = sh.state_dict()
        for k, v in first.state_dict().items():
            if not S.is_table(k):
                assert torch.equal(v, sd[k]), f"rank {r} buffer {k}"
    again, _ = three_steps()
    a, b = ranks.state(), again.state()
    assert sum(S.is_table(k) for k in a) == 14
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert rankops.error_flags() == 0


# ------------------------------------------------------------------ 4. eval after training

def test_eval_after_training_reads_the_updated_weights():
    rows, D, hidden, P, B, seed = S.WECHAT7, 8, [32, 16], 3, 33, 31
    ranks = Ranks(S.initial_model(rows, D, hidden, seed).cuda(), P)
    cats, _ = S.make_batches(rows, P, B, seed=seed)

    def eval_forward():
        def body(r, sh):
            sh.eval()
            with torch.no_grad():
                out = sh({f: t.cuda() for f, t in cats[r].items()})
            sh.train()
            return [o.cpu() for o in out]
        return ranks.run(body)

    def check(outs):
        p = ranks.state()
        for r in range(P):
            with torch.no_grad():
                want = ref.deepfm_forward(p, cats[r], list(rows), len(hidden), True, 0.0)
            for i, (a, b) in enumerate(zip(outs[r], want)):
                torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4, msg=lambda m: f"rank {r} output {i}: {m}")

    check(eval_forward())  # builds the packed table and weight images of the start weights
    start = ranks.state()
    ranks.train_steps([S.make_batches(rows, P, B, seed=seed * 100 + i) for i in range(3)])
    assert any(not torch.equal(v, start[k]) for k, v in ranks.state().items() if S.is_table(k))
    check(eval_forward())
    assert rankops.error_flags() == 0


# ------------------------------------------------------------------ 5. memory

def test_step_allocates_nothing_of_a_tables_size():
    """One 200,000-row field: the peak memory allocated over a step (after the first, which creates
    the moments) stays below one copy of that field's second-order table."""
    rows = dict(S.WECHAT7, userid=200_000)
    full = S.initial_model(rows, 8, [32, 16], 41).cuda()
    sh = ShardedDeepFM.from_deepfm(full).train()
    del full
    opts = sh.optimizers()
    cats, labels = S.make_batches(rows, 1, 33, seed=42)
    cat, label = {f: t.cuda() for f, t in cats[0].items()}, labels[0].cuda()
    sh.train_step(cat, label, opts)
    torch.cuda.synchronize()
    table_bytes = sh.second_order_embeddings["userid"].weight.numel() * 4
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    sh.train_step(cat, label, opts)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak over a sharded step: {peak} bytes; one table copy: {table_bytes} bytes")
    assert peak < table_bytes
    assert rankops.error_flags() == 0


# ------------------------------------------------------------------ 6. API errors

def test_api_errors():
    rows = S.WECHAT7
    sh = ShardedDeepFM.from_deepfm(S.initial_model(rows, 8, [32, 16], 51).cuda()).train()
    cats, labels = S.make_batches(rows, 1, 9, seed=52)
    cat, label = {f: t.cuda() for f, t in cats[0].items()}, labels[0].cuda()

    def backward():
        torch.nn.functional.binary_cross_entropy(sh(cat)[0].reshape(-1), label).backward()

    with pytest.raises(RuntimeError, match="no train backward"):
        sh.sync_gradients()
    backward()
    with pytest.raises(RuntimeError, match="sync_gradients"):
        backward()
    sh.sync_gradients()
    backward()  # consumed: the next step goes through
    sh.sync_gradients()
    six = ShardedDeepFM(rows, embedding_dim=6, hidden_units=[32, 16]).cuda().train()
    with pytest.raises(NotImplementedError, match="embedding_dim % 4"):
        six(cat)
    with torch.no_grad(), pytest.raises(NotImplementedError):  # train mode without autograd: refused as before
        sh(cat)
    wide = {f"f{i:02d}": 5 for i in range(33)}  # 33 fields on one owner, and 17 + 16 on two: both refused by name
    with pytest.raises(NotImplementedError, match="32 fields per owner"):
        ShardedDeepFM(wide, embedding_dim=8, hidden_units=[16]).cuda().train()(
            {f: torch.zeros(2, dtype=torch.int64, device="cuda") for f in wide})
    with pytest.raises(NotImplementedError, match="32 fields in all"):
        ShardedDeepFM(wide, embedding_dim=8, hidden_units=[16], rank=0, world_size=2).cuda().train()(
            {f: torch.zeros(2, dtype=torch.int64, device="cuda") for f in wide})
    # frozen tables get no gradient; frozen dense parameters leave nothing for the backward to hang on
    frozen = sh.second_order_embeddings["userid"].weight.requires_grad_(False)
    for p in sh.parameters():
        p.grad = None
    backward()
    sh.sync_gradients()
    assert frozen.grad is None and sh.first_order_embeddings["userid"].weight.grad.is_sparse
    assert sh.second_order_embeddings["feedid"].weight.grad.is_sparse
    frozen.requires_grad_(True)
    dense = sh.dense_parameters()
    for p in dense:
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="dense"):
        sh(cat)
    for p in dense:
        p.requires_grad_(True)
    sh.eval()
    with torch.no_grad():
        out = sh(cat)
        want = ref.deepfm_forward({k: v.cpu() for k, v in sh.state_dict().items()}, cats[0], list(rows), 2, True, 0.0)
    for a, b in zip(out, want):
        torch.testing.assert_close(a.cpu(), b, rtol=1e-4, atol=1e-4)
    assert rankops.error_flags() == 0
