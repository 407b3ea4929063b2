"""CPU tests of the sparse Adam step: the float64 restatement (tests/sparse_adam_ref.py) against
torch.optim.SparseAdam, the float32 drift the GPU tolerances rest on, and rankops.SparseAdam's
host side (constructor validation, the CPU-parameter error, state dicts moving between it and
torch.optim.SparseAdam)."""
import copy
import inspect

import pytest
import torch

import helpers  # noqa: F401  (puts the package on the path)
import rankops
import sparse_adam_ref as R

f64 = torch.float64


@pytest.mark.parametrize("rows,dim,nnz", [(7, 6, 65), (50, 1, 200), (1000, 32, 4097)])
def test_restatement_is_torch_sparse_adam(rows, dim, nnz):
    """Three consecutive steps with duplicated indices, float64, to 1e-12."""
    g = R.gen("host", rows, dim, nnz)
    p0 = torch.randn(rows, dim, generator=g, dtype=f64)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SparseAdam([ref], lr=R.LR, betas=R.BETAS, eps=R.EPS)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t in range(1, 4):
        idx = torch.randint(0, rows, (nnz,), generator=g)
        vals = torch.rand(nnz, dim, generator=g, dtype=f64) + 0.5  # one sign: no moment cancels to near zero
        assert nnz == 1 or idx.unique().numel() < nnz or rows >= nnz, "duplicates expected"
        ref.grad = torch.sparse_coo_tensor(idx.unsqueeze(0), vals, (rows, dim))
        opt.step()
        R.sparse_adam_step(p, m, v, idx, vals, t)
        st = opt.state[ref]
        for got, want, what in ((p, ref.detach(), "param"), (m, st["exp_avg"], "exp_avg"),
                                (v, st["exp_avg_sq"], "exp_avg_sq")):
            rel, err, scale = R.err_of(what, got, want)
            assert rel <= 1e-12, f"step {t} {what}: {err:.3e} against max {scale:.3e}"


def test_restatement_drops_out_of_range_ids():
    p0 = torch.randn(7, 3, generator=R.gen("oob"), dtype=f64)
    idx = torch.tensor([1, 9, 1, -1, 4])
    vals = torch.rand(5, 3, dtype=f64, generator=R.gen("oob", 1)) + 0.5
    a = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    b = [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)]
    R.sparse_adam_step(*a, idx, vals, 1)
    keep = torch.tensor([0, 2, 4])
    R.sparse_adam_step(*b, idx[keep], vals[keep], 1)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(a[0][[0, 2, 3, 5, 6]], p0[[0, 2, 3, 5, 6]])


def test_float32_drift_sets_the_gpu_tolerances():
    """REL is 50 x DRIFT, and DRIFT is the drift of a float32 run of the restatement on the GPU
    tests' inputs as recorded to three digits: the measurement may not exceed the record, nor fall
    more than 2 % below it (a change of the case table has to be followed by a new record)."""
    worst = R.measure_drift()
    print({k: f"{x:.4e}" for k, x in worst.items()})
    for k, drift in worst.items():
        assert R.REL[k] == R.MARGIN * R.DRIFT[k]
        assert drift <= R.DRIFT[k], f"{k}: measured drift {drift:.4e} above the recorded {R.DRIFT[k]:.3e}"
        assert drift >= 0.98 * R.DRIFT[k], f"{k}: measured drift {drift:.4e}, the recorded {R.DRIFT[k]:.3e} is loose"


def test_per_row_error_sees_a_small_row_beside_a_hot_one():
    want = torch.tensor([[1000.0, 2000.0], [1.0, 0.5]], dtype=f64)
    got = want.clone()
    got[1, 1] += 1e-3
    assert R.rel_err(got, want)[0] == pytest.approx(1e-3 / 2000.0)
    rel, err, scale = R.rel_err(got, want, per_row=True)
    assert rel == pytest.approx(1e-3) and err == pytest.approx(1e-3) and scale == 1.0
    assert R.PER_ROW == {"param": False, "exp_avg": True, "exp_avg_sq": True}
    # the input condition keeps every touched row's moments away from zero, so the per-row scale is sound
    for name in ("padded_history", "d1_r7_n65"):
        case = R.make_case(name)
        for tables in R.run_case(case):
            for t, (_, m, v) in zip(case, tables):
                seen = torch.cat([idx for idx, _ in t["steps"][:1]]).unique()
                assert float(m[seen].abs().min()) >= 0.05 and float(v[seen].min()) >= 2.5e-4


def test_case_table_covers_the_issue():
    names = set(R.CASES)
    for d in (1, 6, 32):
        for r in (1, 7, 1000):
            for n in (1, 63, 64, 65, 4097):
                assert f"d{d}_r{r}_n{n}" in names
    assert any(t["mode"] == "one_row" and t["nnz"] == 8192 for c in R.CASES.values() for t in c)
    assert any(t["idx_stride"] == 2 for c in R.CASES.values() for t in c)
    assert any(t["value_pad"] > 0 for c in R.CASES.values() for t in c)
    assert sorted(t["dim"] for t in R.CASES["three_tables"]) == [1, 6, 32]
    assert any(t["coalesced"] for c in R.CASES.values() for t in c)
    for name in ("distinct", "coalesced"):
        for t in R.make_case(name):
            for idx, _ in t["steps"]:
                assert idx.unique().numel() == idx.numel()
    for t in R.make_case("coalesced"):
        for idx, _ in t["steps"]:
            assert bool((idx[1:] > idx[:-1]).all())


def test_constructor_validation():
    p = [torch.nn.Parameter(torch.zeros(4, 2))]
    with pytest.raises(ValueError, match="learning rate"):
        rankops.SparseAdam(p, lr=0.0)
    with pytest.raises(ValueError, match="epsilon"):
        rankops.SparseAdam(p, eps=0.0)
    with pytest.raises(ValueError, match="beta parameter at index 0"):
        rankops.SparseAdam(p, betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="beta parameter at index 1"):
        rankops.SparseAdam(p, betas=(0.9, -0.1))
    with pytest.raises(NotImplementedError, match="maximize"):
        rankops.SparseAdam(p, maximize=True)
    with pytest.raises(ValueError, match="dense"):
        rankops.SparseAdam([torch.zeros(4, 2).to_sparse().requires_grad_()])
    with pytest.raises(TypeError):
        rankops.SparseAdam(p, 1e-3, (0.9, 0.999), 1e-8, False, True)  # capturable is keyword-only
    opt = rankops.SparseAdam(p, lr=2e-3, betas=(0.8, 0.9), eps=1e-6, capturable=True)
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["maximize"], g["capturable"]) == (2e-3, (0.8, 0.9), 1e-6, False, True)
    assert rankops.SparseAdam(p).param_groups[0]["capturable"] is False
    assert "SparseAdam" in rankops.__all__


def test_cpu_parameter_and_dense_gradient_raise():
    p = torch.nn.Parameter(torch.zeros(4, 2))
    opt = rankops.SparseAdam([p])
    p.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.ones(1, 2), (4, 2))
    with pytest.raises(RuntimeError, match="ROCm"):
        opt.step()
    p.grad = torch.ones(4, 2)
    with pytest.raises(RuntimeError, match="does not support dense gradients"):
        opt.step()
    with pytest.raises(NotImplementedError, match="sparse gradients"):  # rankops.Adam keeps refusing them
        q = torch.nn.Parameter(torch.zeros(4, 2))
        q.grad = torch.sparse_coo_tensor(torch.tensor([[1]]), torch.ones(1, 2), (4, 2))
        rankops.Adam([q]).step()


def test_state_dict_round_trip_with_torch_sparse_adam():
    g = R.gen("state")
    p = torch.nn.Parameter(torch.randn(9, 4, generator=g))
    theirs = torch.optim.SparseAdam([p], lr=3e-3, betas=(0.8, 0.95), eps=1e-7)
    for _ in range(2):
        idx = torch.randint(0, 9, (12,), generator=g)
        p.grad = torch.sparse_coo_tensor(idx.unsqueeze(0), torch.randn(12, 4, generator=g), (9, 4))
        theirs.step()
    sd = copy.deepcopy(theirs.state_dict())
    for capturable in (False, True):
        ours = rankops.SparseAdam([p], capturable=capturable)
        ours.load_state_dict(copy.deepcopy(sd))
        assert ours.param_groups[0]["capturable"] is capturable
        assert ours.param_groups[0]["lr"] == 3e-3 and tuple(ours.param_groups[0]["betas"]) == (0.8, 0.95)
        st = ours.state[p]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and int(st["step"]) == 2
        back = ours.state_dict()
        assert back["state"][0]["step"] == 2 and isinstance(back["state"][0]["step"], int)
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][0][k], sd["state"][0][k])
        again = torch.optim.SparseAdam([p])
        again.load_state_dict(back)
        assert again.state[p]["step"] == 2 and again.param_groups[0]["lr"] == 3e-3
        idx = torch.tensor([[0, 3, 3]])
        p.grad = torch.sparse_coo_tensor(idx, torch.ones(3, 4), (9, 4))
        before = p.detach().clone()
        again.step()  # the loaded state steps on
        assert again.state[p]["step"] == 3 and not torch.equal(before[3], p.detach()[3])
        assert torch.equal(before[1], p.detach()[1])


def test_models_take_sparse_grad_keyword_without_touching_state_dict():
    import sparse_models as M
    for name in M.MODELS:
        a, b = M.build(name, False), M.build(name, True)
        assert a.sparse_grad is False and b.sparse_grad is True, name
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb), name  # same keys in the same creation order
        assert all(torch.equal(sa[k], sb[k]) for k in sa), name
        params = list(inspect.signature(type(a).__init__).parameters.values())
        assert params[-1].name == "sparse_grad" and params[-1].kind is inspect.Parameter.KEYWORD_ONLY, name
        assert params[-1].default is False, name
    # exactly the positional arguments and one more value: refused, the keyword is not positional
    cols = helpers.afm_feature_columns(M.VOCAB)
    assert rankops.AFM(cols, 8, 16).sparse_grad is False
    with pytest.raises(TypeError):
        rankops.AFM(cols, 8, 16, True)
    with pytest.raises(TypeError):
        rankops.FwFM([5, 5, 5, 5, 5, 5], 8, True)


def test_new_struct_layouts_match_the_c_compiler():
    """rk_sparse_adam_tensor and rk_pack_block as ctypes see them against what gcc makes of the header."""
    import ctypes
    import os
    import subprocess
    import tempfile
    from rankops import _lib
    header = os.path.join(helpers.REPO, "include", "rankops.h")
    structs = {"rk_sparse_adam_tensor": _lib.SparseAdamTensor, "rk_pack_block": _lib.PackBlock}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void) {"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(src, "w") as f:
            f.write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-Wall", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {(p[0], p[1]): int(p[2]) for p in (line.split() for line in out) if len(p) == 3}
    for cname, cls in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
