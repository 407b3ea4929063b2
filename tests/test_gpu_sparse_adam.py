"""rk_sparse_adam_step on the GPU against the float64 restatement (tests/sparse_adam_ref.py): every
case of its table as three steps in a row, within REL (50 x the restatement's float32 drift)."""
import pytest
import torch

import helpers  # noqa: F401
import rankops
import sparse_adam_ref as R
from rankops import ops

pytestmark = pytest.mark.gpu


def device_case(case):
    """Device tensors of a case in the layouts its specs ask for."""
    out = []
    for t in case:
        spec = t["spec"]
        p = t["p0"].float().cuda()
        steps = []
        for idx, vals in t["steps"]:
            n, d = vals.shape
            ibuf = torch.full((n * spec["idx_stride"],), -7, dtype=torch.int64, device="cuda")
            ibuf[::spec["idx_stride"]] = idx.cuda()
            vbuf = torch.full((n, d + spec["value_pad"]), float("nan"), device="cuda")
            vbuf[:, :d] = vals.float().cuda()
            steps.append((ibuf[::spec["idx_stride"]], vbuf[:, :d]))
        out.append(dict(spec=spec, p=p, m=torch.zeros_like(p), v=torch.zeros_like(p), steps=steps))
    return out


def run_gpu(case, device_step=None, check=None, keep=None):
    dev = device_case(case)
    ws = None
    for s in range(R.STEPS):
        entries = [(t["p"], t["m"], t["v"], *t["steps"][s], t["spec"]["coalesced"]) for t in dev]
        ws = ops.sparse_adam_step(entries, R.LR, *R.BETAS, R.EPS, 0 if device_step is not None else s + 1,
                                  ops._lib.raw_stream(torch.device("cuda")), device_step=device_step, workspace=ws)
        if check is not None:
            check(s, dev)
    torch.cuda.synchronize()
    if keep is not None:
        keep["workspace"] = ws
    return dev


def assert_close(got, want, what):
    for k, g, w in zip(R.REL, got, want):
        rel, err, scale = R.err_of(k, g, w)
        print(f"{what} {k}: max |err| = {err:.3e}, max |want| = {scale:.3e}")
        assert rel <= R.REL[k], f"{what} {k}: {err:.3e} > {R.REL[k]} * {scale:.3e}"


@pytest.mark.parametrize("name", list(R.CASES))
def test_three_steps_match_the_restatement(name):
    case = R.make_case(name)
    want = R.run_case(case)

    def check(s, dev):
        for k, t in enumerate(dev):
            assert_close((t["p"], t["m"], t["v"]), want[s][k], f"{name} step {s + 1} table {k}")

    dev = run_gpu(case, check=check)
    assert rankops.error_flags() == 0
    # rows absent from every step's gradient: bit-identical parameter, moments never written
    for t, d in zip(case, dev):
        seen = torch.zeros(t["spec"]["rows"], dtype=torch.bool)
        for idx, _ in t["steps"]:
            seen[idx] = True
        assert torch.equal(d["p"].cpu()[~seen], t["p0"].float()[~seen])
        assert not d["m"].cpu()[~seen].any() and not d["v"].cpu()[~seen].any()
        assert bool((d["p"].cpu()[seen] != t["p0"].float()[seen]).any(1).all()), "every row in the gradient moved"


@pytest.mark.parametrize("name", ["three_tables", "one_row_n8192", "padded_history", "coalesced_and_sorted"])
def test_repeated_call_is_bit_equal(name):
    case = R.make_case(name)
    a, b = run_gpu(case), run_gpu(case)
    for x, y in zip(a, b):
        for k in ("p", "m", "v"):
            assert torch.equal(x[k], y[k]), k


def test_rows_absent_from_one_step_keep_their_bits():
    """Per step: rows outside that step's gradient keep parameter and both moments bit for bit."""
    case = R.make_case("d6_r1000_n65")
    prev = {}

    def check(s, dev):
        t = dev[0]
        cur = {k: t[k].clone() for k in ("p", "m", "v")}
        if prev:
            absent = torch.ones(1000, dtype=torch.bool)
            absent[case[0]["steps"][s][0]] = False
            for k in cur:
                assert torch.equal(cur[k].cpu()[absent], prev[k].cpu()[absent]), k
        prev.update(cur)

    run_gpu(case, check=check)


@pytest.mark.parametrize("name", ["three_tables", "coalesced", "d32_r7_n4097"])
def test_device_step_counter_equals_host_step(name):
    """Both forms make the step size in double and round it once, so it may differ by one ulp of
    the device's pow at the most: the scalar the device wrote is held to that, and so is every
    parameter element (an off-by-one in the device count would move the scalar by 30 %)."""
    case = R.make_case(name)
    host = run_gpu(case)
    counter = torch.zeros((), device="cuda")
    keep = {}
    dev = run_gpu(case, device_step=counter, keep=keep)
    assert float(counter) == R.STEPS
    b1, b2 = R.BETAS
    step_size = torch.tensor(R.LR * (1 - b2 ** R.STEPS) ** 0.5 / (1 - b1 ** R.STEPS), dtype=torch.float64).float()
    on_device = keep["workspace"][:4].view(torch.float32).cpu()[0]  # the step-size slot of the workspace
    ulp = float(torch.finfo(torch.float32).eps) * float(step_size)
    print(f"{name}: step size host {float(step_size):.9e}, device {float(on_device):.9e}")
    assert abs(float(on_device) - float(step_size)) <= ulp
    want = R.run_case(case)[-1]
    for x, y, w in zip(dev, host, want):
        assert_close((x["p"], x["m"], x["v"]), w, f"{name} device step")
        assert torch.equal(x["m"], y["m"]) and torch.equal(x["v"], y["v"])  # the moments do not see the count
        # p -= step_size * ratio with |ratio| < 4 here: per step one ulp of the scalar, and one
        # rounding of p where the two differ
        diff = (x["p"].double() - y["p"].double()).abs()
        bound = R.STEPS * (4 * ulp + torch.finfo(torch.float32).eps * y["p"].double().abs())
        assert bool((diff <= bound).all()), f"{name}: max diff {float(diff.max()):.3e}"


def test_out_of_range_id_raises_the_flag_and_leaves_the_rest_correct():
    case = R.make_case("three_tables")
    for t in case:
        rows = t["spec"]["rows"]
        for idx, _ in t["steps"]:
            idx[0], idx[idx.numel() // 2], idx[-1] = rows, -1, rows + 12345
    want = R.run_case(case)  # the restatement drops them
    rankops.error_flags()
    dev = run_gpu(case)
    assert rankops.error_flags() & 1
    for k, t in enumerate(dev):
        assert_close((t["p"], t["m"], t["v"]), want[-1][k], f"oob table {k}")
    clean = run_gpu(R.make_case("d1_r7_n63"))
    assert rankops.error_flags() == 0 and clean


def test_argument_validation():
    lib = ops._lib.load()
    p = torch.zeros(4, 2, device="cuda")
    idx = torch.zeros(3, dtype=torch.int64, device="cuda")
    val = torch.ones(3, 2, device="cuda")
    arr = ops.sparse_adam_tensors([(p, p.clone(), p.clone(), idx, val, False)])
    arr[0].rows = 1 << 32
    import ctypes
    nbytes = ctypes.c_int64()
    assert lib.rk_sparse_adam_step_workspace_size(arr, 1, ctypes.byref(nbytes)) == ops._lib.RK_ERR_UNSUPPORTED
    arr[0].rows = 4
    assert lib.rk_sparse_adam_step_workspace_size(arr, 1, ctypes.byref(nbytes)) == 0 and nbytes.value > 0
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    st = ops._lib.raw_stream(torch.device("cuda"))
    assert lib.rk_sparse_adam_step(arr, 1, 1e-3, 0.9, 0.999, 1e-8, 1, None, ws.data_ptr(), 16, st) == 1  # workspace
    assert lib.rk_sparse_adam_step(arr, 1, 1e-3, 0.9, 0.999, 1e-8, 0, None, ws.data_ptr(), ws.numel(), st) == 1
    assert lib.rk_sparse_adam_step(arr, 1, 1e-3, 1.0, 0.999, 1e-8, 1, None, ws.data_ptr(), ws.numel(), st) == 1
    torch.cuda.synchronize()
    assert not p.any()


@pytest.mark.parametrize("capturable", [False, True])
def test_plain_sparse_embedding_is_stepped_like_torch(capturable):
    """nn.Embedding(sparse=True) under torch autograd, rankops.SparseAdam on the GPU against
    torch.optim.SparseAdam on a float64 CPU twin; then the state dict moves to torch's class."""
    g = R.gen("plain embedding")
    emb = torch.nn.Embedding(50, 6, sparse=True)
    twin = torch.nn.Embedding(50, 6, sparse=True).double()
    twin.weight.data.copy_(emb.weight.data)
    emb = emb.cuda()
    ours = rankops.SparseAdam(emb.parameters(), lr=R.LR, betas=R.BETAS, eps=R.EPS, capturable=capturable)
    theirs = torch.optim.SparseAdam(twin.parameters(), lr=R.LR, betas=R.BETAS, eps=R.EPS)
    sign = torch.randint(0, 2, (50, 6), generator=g).double() * 2 - 1
    for step in range(R.STEPS):
        ids = torch.randint(0, 50, (33, 3), generator=g)
        w = sign[ids] * (torch.rand(33, 3, 6, generator=g, dtype=torch.float64) + 0.5)  # the input condition
        ours.zero_grad()
        theirs.zero_grad()
        (emb(ids.cuda()) * w.float().cuda()).sum().backward()
        (twin(ids) * w).sum().backward()
        assert emb.weight.grad.is_sparse and not emb.weight.grad.is_coalesced()
        version = emb.weight._version
        ours.step()
        theirs.step()
        assert emb.weight._version > version
        st, ref = ours.state[emb.weight], theirs.state[twin.weight]
        assert_close((emb.weight, st["exp_avg"], st["exp_avg_sq"]),
                     (twin.weight, ref["exp_avg"], ref["exp_avg_sq"]), f"plain embedding step {step + 1}")
    # a coalesced gradient goes in with the flag set
    ids = torch.randperm(50, generator=g)[:20]
    vals = sign[ids] * (torch.rand(20, 6, generator=g, dtype=torch.float64) + 0.5)
    emb.weight.grad = torch.sparse_coo_tensor(ids.unsqueeze(0).cuda(), vals.float().cuda(), (50, 6)).coalesce()
    twin.weight.grad = torch.sparse_coo_tensor(ids.unsqueeze(0), vals, (50, 6))
    assert emb.weight.grad.is_coalesced()
    ours.step()
    theirs.step()
    st, ref = ours.state[emb.weight], theirs.state[twin.weight]
    assert_close((emb.weight, st["exp_avg"], st["exp_avg_sq"]), (twin.weight, ref["exp_avg"], ref["exp_avg_sq"]),
                 "coalesced gradient")
    sd = ours.state_dict()
    assert sd["state"][0]["step"] == R.STEPS + 1 and isinstance(sd["state"][0]["step"], int)
    moved = torch.optim.SparseAdam(emb.parameters())
    moved.load_state_dict(sd)
    assert moved.state[emb.weight]["step"] == R.STEPS + 1
    assert torch.equal(moved.state[emb.weight]["exp_avg"], st["exp_avg"])
    assert rankops.error_flags() == 0


def _two_tables(seed):
    g = R.gen("state dict", seed)
    return [torch.nn.Parameter(torch.randn(40, 6, generator=g).cuda()), torch.nn.Parameter(torch.randn(9, 1, generator=g).cuda())]


def _grads(tables, step):
    g = R.gen("state dict grads", step)
    for p in tables:
        ids = torch.randint(0, p.shape[0], (50,), generator=g)
        p.grad = torch.sparse_coo_tensor(ids.unsqueeze(0).cuda(), (torch.rand(50, p.shape[1], generator=g) + 0.5).cuda(),
                                         p.shape)


def test_state_dict_between_capturable_steps_leaves_the_live_counter_alone():
    """Three capturable steps, state_dict(), three more: the live device counter is the same object
    throughout, shared by both tables (one call per step), and the result equals an uninterrupted
    run bit for bit.  The dict holds torch's ints and loads into torch.optim.SparseAdam."""
    runs = []
    for interrupt in (False, True):
        tables = _two_tables(3)
        opt = rankops.SparseAdam(tables, lr=R.LR, capturable=True)
        counter = None
        for step in range(6):
            _grads(tables, step)
            opt.step()
            live = [opt.state[p]["step"] for p in tables]
            assert live[0] is live[1] and isinstance(live[0], torch.Tensor) and live[0].is_cuda
            counter = counter if counter is not None else live[0]
            assert live[0] is counter
            if interrupt and step == 2:
                sd = opt.state_dict()
                assert [sd["state"][k]["step"] for k in (0, 1)] == [3, 3]
                assert opt.state[tables[0]]["step"] is counter and float(counter) == 3.0
                assert sd["state"][0]["exp_avg"] is opt.state[tables[0]]["exp_avg"]
                theirs = torch.optim.SparseAdam(tables, lr=R.LR)
                theirs.load_state_dict(sd)
                assert theirs.state[tables[1]]["step"] == 3
        assert float(counter) == 6.0
        runs.append([p.detach().clone() for p in tables] + [opt.state[p]["exp_avg_sq"].clone() for p in tables])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_state_dict_between_graph_replays():
    """The same with the step captured: a checkpoint between replays must not take the counter the
    graph writes to away from the optimizer."""
    runs = []
    for interrupt in (False, True):
        tables = _two_tables(4)
        opt = rankops.SparseAdam(tables, lr=R.LR, capturable=True)
        _grads(tables, 0)
        grads = [p.grad for p in tables]
        opt.step()
        counter = opt.state[tables[0]]["step"]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            opt.step()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            opt.step()
        for replay in range(4):
            g.replay()
            if interrupt and replay == 1:
                torch.cuda.synchronize()
                sd = opt.state_dict()
                assert sd["state"][0]["step"] == 4 and sd["state"][1]["step"] == 4
                junk = [torch.full((), -1000.0, device="cuda") for _ in range(64)]  # would land on a freed counter
        torch.cuda.synchronize()
        assert opt.state[tables[0]]["step"] is counter and opt.state[tables[1]]["step"] is counter
        assert float(counter) == 6.0 and opt.state_dict()["state"][1]["step"] == 6
        runs.append([p.detach().clone() for p in tables])
        del grads
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_loaded_counts_share_one_counter_and_a_missing_gradient_leaves_it():
    tables = _two_tables(5)
    theirs = torch.optim.SparseAdam(tables, lr=R.LR)
    for step in range(2):
        _grads(tables, step)
        theirs.step()
    opt = rankops.SparseAdam(tables, lr=R.LR, capturable=True)
    opt.load_state_dict(theirs.state_dict())
    _grads(tables, 2)
    opt.step()
    a, b = (opt.state[p]["step"] for p in tables)
    assert a is b and float(a) == 3.0  # resumed at count 2: one counter, one call
    _grads(tables, 3)
    tables[1].grad = None  # torch counts a parameter's steps only when it has a gradient
    before = tables[1].detach().clone()
    opt.step()
    a, b = (opt.state[p]["step"] for p in tables)
    assert a is not b and float(a) == 4.0 and float(b) == 3.0
    assert torch.equal(tables[1].detach(), before)
    assert [opt.state_dict()["state"][k]["step"] for k in (0, 1)] == [4, 3]
    # against torch from the same state: the second table's next step is its fourth
    twin = [torch.nn.Parameter(p.detach().double().cpu()) for p in tables]
    ref = torch.optim.SparseAdam(twin, lr=R.LR)
    sd = opt.state_dict()
    for st in sd["state"].values():
        st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"].double().cpu(), st["exp_avg_sq"].double().cpu()
    ref.load_state_dict(sd)
    _grads(tables, 4)
    for p, q in zip(tables, twin):
        q.grad = torch.sparse_coo_tensor(p.grad._indices().cpu(), p.grad._values().double().cpu(), p.shape)
    opt.step()
    ref.step()
    for p, q in zip(tables, twin):
        rel, err, scale = R.rel_err(p, q)
        assert rel <= R.REL["param"], f"{err:.3e} against {scale:.3e}"
