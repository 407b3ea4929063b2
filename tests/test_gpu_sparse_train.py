"""sparse_grad=True on all eight models: the sparse COO table gradients against the dense ones of
the same engine, a step of rankops.Adam (dense parameters) + rankops.SparseAdam (tables), the
step as a hipGraph, and the memory a sparse step allocates."""
import pytest
import torch

import helpers as H
import rankops
import sparse_models as M

pytestmark = pytest.mark.gpu


def twins(name, vocab=M.VOCAB):
    """(dense model, sparse model) on the GPU in train mode with equal weights and, for the models
    that draw interaction weights, equal frozen draws."""
    dense, sparse = M.build(name, False, vocab).cuda().train(), M.build(name, True, vocab).cuda().train()
    sparse.load_state_dict(dense.state_dict())
    assert sparse.sparse_grad and not dense.sparse_grad
    return dense, sparse


def backward(model, name, inp, label, seed=5):
    torch.manual_seed(seed)  # the dropout streams' seed and the frozen interaction weights' draw
    model.zero_grad(set_to_none=True)
    loss = M.loss_of(model, name, inp, label)
    loss.backward()
    return loss.detach()


def split(model):
    tables = [p for p in model.parameters() if M.is_table(model, p)]
    rest = [p for p in model.parameters() if not M.is_table(model, p)]
    return tables, rest


@pytest.mark.parametrize("name", M.MODELS)
def test_sparse_gradients_equal_the_dense_ones(name):
    dense, sparse = twins(name)
    inp = H.to_device(M.inputs(name), "cuda")
    label = M.labels().cuda()
    la, lb = backward(dense, name, inp, label), backward(sparse, name, inp, label)
    torch.testing.assert_close(la, lb, rtol=1e-6, atol=1e-6)
    tables = 0
    for (n, a), b in zip(dense.named_parameters(), sparse.parameters()):
        if a.grad is None:
            assert b.grad is None, n
            continue
        if M.is_table(dense, a):
            tables += 1
            g = b.grad
            assert g.is_sparse and not g.is_coalesced() and g.shape == a.shape, n
            assert g._values().shape[1:] == a.shape[1:] and g._indices().shape[0] == 1, n
            want = a.grad
            scale = max(1e-3, float(want.abs().max()))
            # the tolerance of tests/test_gpu_train.py for embedding gradients
            torch.testing.assert_close(g.to_dense(), want, rtol=0, atol=2e-4 * scale, msg=lambda m: f"{n}: {m}")
        else:  # the same kernels ran; some reduce with float atomics (AFM's pooling, the split-K
            # weight gradients), so two runs agree to summation order: test_gpu_train.py's gradient bound
            assert not b.grad.is_sparse, n
            scale = max(1e-3, float(a.grad.abs().max()))
            torch.testing.assert_close(b.grad, a.grad, rtol=0, atol=2e-4 * scale, msg=lambda m: f"{n}: {m}")
    assert tables >= 5
    assert rankops.error_flags() == 0


def test_history_lookups_stay_in_the_list_and_shared_tables_get_one_gradient():
    """DIEN feeds the feedid table from the target lookup and the history (its auxiliary loss adds
    the negatives): one gradient, nnz = all lookups, entries concatenated.  DIN keeps the history in
    a table of its own, BST's feedid table is fed by the history alone.  Padded positions stay in
    the list; their values are exactly zero in DIN and DIEN."""
    n_hist = M.B * M.T
    for name, nnz in (("din", n_hist), ("bst", n_hist), ("dien", M.B + n_hist),
                      ("dien_aux", M.B + n_hist + M.B * (M.T - 1) * M.T_NEG)):
        _, sparse = twins(name)
        raw = M.inputs(name)
        backward(sparse, name, H.to_device(raw, "cuda"), M.labels().cuda())
        g = sparse.embeddings["his_read_comment_7d_seq" if name == "din" else "feedid"].weight.grad
        assert g.is_sparse and g._nnz() == nnz, name
        ids = g._indices()[0].cpu()
        if name == "bst":
            assert torch.equal(ids, raw["seq_feedid"].reshape(-1))  # the category row holds no feedid lookup
            continue
        seq = raw["sequence"]["his_read_comment_7d_seq"]
        lens = raw["sequence"]["his_read_comment_7d_seq_length"]
        first = 0 if name == "din" else M.B
        if first:
            assert torch.equal(ids[:M.B], raw["target"]["feedid"]), name
        assert torch.equal(ids[first:first + n_hist], seq.reshape(-1)), name
        if name == "dien_aux":
            # the negatives of steps past a sample's length arrive as id 0 with an exactly zero row
            neg, got = raw["sequence"][M.NEG_KEY].reshape(-1), ids[first + n_hist:]
            masked = got != neg
            assert bool((got[masked] == 0).all()) and not g._values()[first + n_hist:].cpu()[masked].any(), name
            assert not masked.all(), name
        past = (torch.arange(M.T)[None, :] >= lens[:, None]).reshape(-1)
        assert past.any() and not g._values()[first:first + n_hist].cpu()[past].any(), name


@pytest.mark.parametrize("name", M.MODELS)
def test_value_rows_are_packed_by_one_launch_per_backward(name, monkeypatch):
    """All of a model's tables, BST's position tables included, in one rk_pack_blocks call."""
    from rankops import ops
    calls = []
    real = ops.pack_blocks
    monkeypatch.setattr(ops, "pack_blocks", lambda blocks, stream: (calls.append(len(blocks)), real(blocks, stream))[1])
    _, sparse = twins(name)
    backward(sparse, name, H.to_device(M.inputs(name), "cuda"), M.labels().cuda())
    tables = sum(p.grad is not None and p.grad.is_sparse for p in sparse.parameters())
    assert len(calls) == 1 and calls[0] >= tables >= 5, (calls, tables)
    if name == "bst2":
        for blk in sparse.transformer_blocks:
            g = blk.position_embedding.weight.grad
            assert g.is_sparse and g._nnz() == M.B * M.T
            assert torch.equal(g._indices()[0].cpu(), torch.arange(M.T).repeat(M.B))


def optimizers(model, capturable=False):
    tables, rest = split(model)
    return (rankops.Adam(rest, lr=1e-3, capturable=capturable),
            rankops.SparseAdam(tables, lr=1e-3, capturable=capturable))


@pytest.mark.parametrize("name", M.MODELS)
def test_one_step_moves_only_the_rows_of_the_batch(name):
    _, model = twins(name)
    raw = M.inputs(name)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opts = optimizers(model)
    backward(model, name, H.to_device(raw, "cuda"), M.labels().cuda())
    grads = {n: p.grad for n, p in model.named_parameters() if p.grad is not None and p.grad.is_sparse}
    for o in opts:
        o.step()
    torch.cuda.synchronize()
    outside = 0
    for n, g in grads.items():
        p = dict(model.named_parameters())[n].detach()
        inside = torch.zeros(p.shape[0], dtype=torch.bool, device="cuda")
        inside[g._indices()[0]] = True
        assert inside.any(), n
        outside += int((~inside).sum())  # a two-row table (device) can lie in the batch as a whole
        assert torch.equal(p[~inside], before[n][~inside]), f"{n}: a row outside the batch changed"
        dense_g = g.to_dense()
        live = inside & (dense_g != 0).any(1)  # a row whose entries are all exact zeros (padding) stays
        assert live.any() and bool((p[live] != before[n][live]).any(1).all()), f"{n}: a row of the batch stayed"
    assert outside > 0 and len(grads) >= 5
    assert rankops.error_flags() == 0


@pytest.mark.parametrize("name", ["deepfm", "dien", "dien_aux"])
def test_graph_replay_equals_eager_steps_bit_for_bit(name):
    """One captured step (forward, backward, rankops.Adam on the dense parameters, rankops.SparseAdam
    on the tables, both capturable) replayed three times against three eager steps of a twin."""
    inp = H.to_device(M.inputs(name), "cuda")
    label = M.labels().cuda()
    results = []
    for mode in ("eager", "graph"):
        torch.manual_seed(0)
        model = M.build(name, True).cuda().train()
        opts = optimizers(model, capturable=True)

        def step():
            for o in opts:
                o.zero_grad(set_to_none=True)
            M.loss_of(model, name, inp, label).backward()
            for o in opts:
                o.step()

        step()  # creates the optimizer states and the workspace
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream().wait_stream(s)
        if mode == "eager":
            for _ in range(3):
                step()
        else:
            for o in opts:
                o.zero_grad(set_to_none=True)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            for _ in range(3):
                g.replay()
        torch.cuda.synchronize()
        results.append({n: t.detach().cpu().clone() for n, t in model.named_parameters()})
    tables = 0
    for n in results[0]:
        tables += "embedding" in n
        diff = float((results[0][n].double() - results[1][n].double()).abs().max())
        print(f"{name} {n}: max |graph - eager| = {diff:.3e}")
    for n in results[0]:
        assert torch.equal(results[0][n], results[1][n]), n
    assert tables >= 5
    assert rankops.error_flags() == 0


def test_sparse_step_allocates_nothing_of_a_tables_size():
    """A 200,000-row table: the peak memory allocated over a sparse step stays below one copy of
    that table (the dense step allocates its gradient and fills it)."""
    vocab = dict(M.VOCAB, userid=200_000)
    model = M.build("dcn", True, vocab).cuda().train()
    inp = H.to_device(M.inputs("dcn", vocab), "cuda")
    label = M.labels().cuda()
    opts = optimizers(model)

    def step():
        for o in opts:
            o.zero_grad(set_to_none=True)
        M.loss_of(model, "dcn", inp, label).backward()
        for o in opts:
            o.step()

    step()  # the optimizer states (two table-sized moments) and the workspace exist from here on
    torch.cuda.synchronize()
    table_bytes = model.embeddings["userid"].weight.numel() * 4
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak over a sparse step: {peak} bytes; one table copy: {table_bytes} bytes")
    assert peak < table_bytes
