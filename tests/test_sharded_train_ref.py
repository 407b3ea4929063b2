"""CPU tests of tests/sharded_train_ref.py, the float64 oracle of test_gpu_sharded_train.py.

The wire restatement (pack indices, split gather, assemble, backward-pack with scale 1/P, unpack) is
tied to autograd: pushed through the same reference forward, the per-table index_add_ of its (ids,
values) must equal the table gradients of the mean-over-ranks loss at 1e-12 relative (close12 of
test_train_ops_ref.py), for P in {1, 2, 3, 4, 8} over seven fields (P = 8: an owner without fields).
At P = 1 the restatement is plain single-model autograd.  Last, the seed condition of the GPU file's
parameter rule: the restatement in float32 against float64 stays inside the 0.5 % cap."""
import pytest
import torch
import torch.nn.functional as F

import sharded_train_ref as S
import train_ops_ref as R
from oracle import reference_forward as ref

f64 = torch.float64
HIDDEN, D, B = [32, 16], 8, 5


def close12(got, want, what):
    assert got.shape == want.shape and got.dtype == f64 and want.dtype == f64, what
    rel, err, scale = R.rel_err(got, want)
    assert rel <= 1e-12, f"{what}: {err:.3e} against max {scale:.3e}"


def wire_step(tr, cats, labels):
    """The sharded data path in float64 around the reference tail: per table (ids, values) at the
    owners, and the per-rank outputs."""
    P, fields = tr.P, tr.fields
    Fn = len(fields)
    owners = S.fields_of(Fn, P)
    p = {k: v.detach() for k, v in tr.p.items()}
    sends = [S.pack_indices([cats[s][f] for f in fields], P) for s in range(P)]
    recv_idx = S.all_to_all(sends, [[B * len(owners[r]) for r in range(P)]] * P)
    rows = []
    for r in range(P):
        t2 = [p[f"second_order_embeddings.{fields[f]}.weight"] for f in owners[r]]
        t1 = [p[f"first_order_embeddings.{fields[f]}.weight"] for f in owners[r]]
        rows.append(S.gather_split(recv_idx[r], t2, t1, P, B) if owners[r] else torch.empty(0, dtype=f64))
    back = [[S.block(B, len(owners[r]), D)] * P for r in range(P)]
    recv_rows = S.all_to_all(rows, back)
    grads, outs = [], []
    for s in range(P):
        deep_in, fm1, fm2 = S.assemble(recv_rows[s], Fn, P, D, B)
        # the reference forward over "tables" that are this rank's assembled rows, looked up at 0..B-1;
        # fm1 rides on the first field's first-order table
        e = deep_in.view(B, Fn, D).clone().requires_grad_(True)
        w1 = fm1.view(B, 1).clone().requires_grad_(True)
        q = {k: v for k, v in p.items() if not S.is_table(k)}
        q.update({k: v.clone() for k, v in tr.buf.items()})
        for i, f in enumerate(fields):
            q[f"second_order_embeddings.{f}.weight"] = e[:, i]
            q[f"first_order_embeddings.{f}.weight"] = w1 if i == 0 else torch.zeros(B, 1, dtype=f64)
        out = ref.deepfm_forward_train(q, {f: torch.arange(B) for f in fields}, fields, tr.nh, tr.bn, tr.dropout, None)
        close12(out[3].detach().view(-1), fm2, f"fm2 of rank {s}")
        loss = F.binary_cross_entropy(out[0].reshape(-1), labels[s].to(f64))
        d_e, dfm1 = torch.autograd.grad(loss, [e, w1])
        grads.append(S.backward_pack(d_e.reshape(B, Fn * D), dfm1.view(B), 1.0 / P, Fn, P, D, B))
        outs.append(out)
    fwd = [[S.block(B, len(owners[r]), D) for r in range(P)]] * P
    recv_g = S.all_to_all(grads, fwd)
    tables = {}
    for r in range(P):
        if not owners[r]:
            assert recv_g[r].numel() == 0
            continue
        ids, v2, v1 = S.unpack(recv_g[r], recv_idx[r], len(owners[r]), D, P, B)
        for j, f in enumerate(owners[r]):
            tables[f"second_order_embeddings.{fields[f]}.weight"] = (ids[j], v2[j])
            tables[f"first_order_embeddings.{fields[f]}.weight"] = (ids[j], v1.view(-1, 1))
    return tables, outs


@pytest.mark.parametrize("P", [1, 2, 3, 4, 8])
def test_wire_restatement_carries_the_autograd_table_gradients(P):
    model = S.initial_model(S.WECHAT7, D, HIDDEN, seed=20 + P)
    tr = S.RefTrainer(model.state_dict(), S.WECHAT7, HIDDEN, P)
    cats, labels = S.make_batches(S.WECHAT7, P, B, seed=30 + P)
    outs, _ = tr.forward_backward(cats, labels)
    before = {k: v.clone() for k, v in tr.buf.items()}
    tables, wire_outs = wire_step(tr, cats, labels)
    assert set(tables) == set(tr.tables)
    for k, (ids, vals) in tables.items():
        assert ids.dtype == torch.int64 and ids.numel() == P * B
        got = torch.zeros_like(tr.p[k].detach()).index_add_(0, ids, vals)
        close12(got, tr.p[k].grad, f"P={P} {k}")
    for s in range(P):
        for i, (a, b) in enumerate(zip(wire_outs[s], outs[s])):
            close12(a.detach(), b.detach(), f"P={P} rank {s} output {i}")
    for k in before:  # wire_step worked on copies
        assert torch.equal(before[k], tr.buf[k])


def test_one_rank_restatement_is_plain_autograd():
    model = S.initial_model(S.WECHAT7, D, HIDDEN, seed=5)
    sd = model.state_dict()
    tr = S.RefTrainer(sd, S.WECHAT7, HIDDEN, 1)
    cats, labels = S.make_batches(S.WECHAT7, 1, B, seed=6)
    outs, losses = tr.forward_backward(cats, labels)
    p = {k: (v.detach().to(f64).requires_grad_(True) if v.is_floating_point() and not k.endswith(
        ("running_mean", "running_var")) else (v.detach().to(f64) if v.is_floating_point() else v.detach().clone()))
         for k, v in sd.items()}
    out = ref.deepfm_forward_train(p, cats[0], list(S.WECHAT7), len(HIDDEN), True, 0.0, None)
    F.binary_cross_entropy(out[0].reshape(-1), labels[0].to(f64)).backward()
    for k in tr.p:
        close12(tr.p[k].grad, p[k].grad, k)
    for k in tr.buf:
        assert torch.equal(tr.buf[k], p[k]), k
    for a, b in zip(outs[0], out):
        close12(a.detach(), b.detach(), "output")


@pytest.mark.parametrize("name", list(S.CONFIGS))
def test_seeds_keep_float32_inside_the_parameter_rule(name):
    """Three steps of RefTrainer in float32 against float64, the float32 run re-synchronised to the
    float64 one after each step: every parameter (tables: the rows of the global batch) inside the
    rule of _assert_adam_params_close, rows outside the batch untouched."""
    rows, dim, hidden, P, Bl, seed = S.CONFIGS[name]
    sd = S.initial_model(rows, dim, hidden, seed).state_dict()
    hi, lo = S.RefTrainer(sd, rows, hidden, P), S.RefTrainer(sd, rows, hidden, P, dtype=torch.float32)
    skip = S.bn_fed_biases(sd)
    worst = 0.0
    for step in range(3):
        cats, labels = S.make_batches(rows, P, Bl, seed=seed * 100 + step)
        prev = lo.state()
        for tr in (hi, lo):
            tr.forward_backward(cats, labels)
            tr.step(cats)
        touched = hi.batch_rows(cats)
        for k in hi.p:
            got, want = lo.p[k].detach(), hi.p[k].detach()
            if k in touched:
                mask = torch.zeros(got.shape[0], dtype=torch.bool)
                mask[touched[k]] = True
                assert torch.equal(got[~mask], prev[k][~mask]), f"{k}: rows outside the batch moved"
                got, want = got[mask], want[mask]
            if k not in skip:
                worst = max(worst, S.adam_rule(got, want, S.LR, f"{name} step {step} {k}"))
        lo.load(hi.state(), *hi.moments())
    print(f"{name}: largest share outside the inner bound {worst:.4%}")
