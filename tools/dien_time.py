"""DIEN at the reference shape (B 4096, T 50, H 16, nh 8, WeChat vocabulary), both cells: the time
of one rk_dien_interest launch, of the whole rankops.DIEN eval forward, and — the baseline, what a
user has without the kernel — of the same forward written as eager torch ops on the same GPU in
the same process (the per-step loop of tests/dien_ref.py in fp32).  Then the train step of
rankops.DIEN(trainable=True): forward + backward + rankops.Adam, eager and as one hipGraph, against
that loop with a train-mode tail differentiated by torch autograd (torch.optim.Adam, fused).
`--aux` runs only the auxiliary-loss leg: the graph-replayed train step without and with
use_auxiliary_loss (3 negatives per step), and the rk_dien_aux_loss / rk_dien_aux_loss_backward
launches alone.

Device times are HIP events around hipGraph replays (the host's launch cost excluded); the eager
loop is timed both as it runs (host clock around a synchronise: its ~1,300 launches are
host-bound) and captured in a graph.  The shader clock the device reports is printed beside them.
Needs a GPU; prints one JSON line at the end."""
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (sets sys.path for rankops and tests/)
import torch  # noqa: E402

import dien_ref  # noqa: E402
import helpers as H  # noqa: E402
import rankops  # noqa: E402
from rankops import _lib, ops  # noqa: E402

B, T = 4096, 50


def shader_clock():
    """The active sclk level the driver reports (read-only sysfs), or None."""
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            for line in open(path):
                if line.strip().endswith("*"):
                    return line.split(":", 1)[1].strip(" *\n")
        except OSError:
            pass
    return None


def grad_graph_of(fn):
    """bench.graph_of with grad mode left on (a whole train step: forward, backward, optimizer)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def graph_avg_ms(fn, iters=20, grad=False):
    g = grad_graph_of(fn) if grad else bench.graph_of(fn)[0]
    st = torch.cuda.current_stream()
    g.replay()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(st)
    for _ in range(iters):
        g.replay()
    end.record(st)
    end.synchronize()
    return start.elapsed_time(end) / iters


def host_avg_ms(fn, iters=5):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def train_step_times(cell, inp):
    """Engine train step (eager call and hipGraph replay) and the eager-autograd baseline, in us."""
    import torch.nn.functional as F
    args = (inp["dense"], inp["category"], inp["sequence"], inp["target"])
    label = (torch.rand(B, device="cuda") < 0.3).float()
    crit = torch.nn.BCELoss()
    out = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(0)
        m = rankops.DIEN(None, custom_gru_type=cell, vocab_sizes=H.WECHAT_VOCAB, trainable=True).cuda().train()
        opt = rankops.Adam(m.parameters(), lr=1e-3, capturable=(mode == "graph"))

        def step():
            opt.zero_grad(set_to_none=False)
            prob, _ = m(*args)
            crit(prob.squeeze(), label).backward()
            opt.step()

        step()  # allocates gradients and optimizer state
        torch.cuda.synchronize()
        if mode == "eager":
            out["train_step_eager_us"] = 1e3 * host_avg_ms(step, iters=20)
        else:
            out["train_step_graph_us"] = 1e3 * graph_avg_ms(step, iters=20, grad=True)
    # baseline: the dien_ref loop + a train-mode tail as torch ops, autograd, torch.optim.Adam
    torch.manual_seed(0)
    m = rankops.DIEN(None, custom_gru_type=cell, vocab_sizes=H.WECHAT_VOCAB).cuda().train()
    p = dict(m.named_parameters())
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, fused=True)
    seq = inp["sequence"]

    def torch_step():
        opt.zero_grad(set_to_none=False)
        cols = [v.reshape(-1, 1) for v in inp["dense"].values()]
        cols += [m.embeddings[f](inp["category"][f]) for f in dien_ref.CATEGORY if f in inp["category"]]
        e_target = m.embeddings["feedid"](inp["target"]["feedid"])
        state, _, _ = dien_ref.interest(e_target, m.embeddings["feedid"](seq[dien_ref.SEQ_KEY]),
                                        seq[f"{dien_ref.SEQ_KEY}_length"], m.interest_weights(), cell,
                                        dtype=torch.float32)
        x = torch.cat(cols + [e_target, state], 1)
        for layer in m.fcn:
            if isinstance(layer, rankops.din.Dice):  # Dice with batch statistics as torch ops
                g = torch.sigmoid(F.batch_norm(x, layer.bn.running_mean, layer.bn.running_var, None, None, True,
                                               layer.bn.momentum, 1e-5))
                x = layer.alpha * (1 - g) * x + g * x
            else:
                x = layer(x)
        crit(torch.sigmoid(m.output_layer(x)).squeeze(), label).backward()
        opt.step()

    torch_step()
    torch.cuda.synchronize()
    out["torch_autograd_step_eager_us"] = 1e3 * host_avg_ms(torch_step, iters=3)
    out["torch_step_over_train_step_eager"] = out["torch_autograd_step_eager_us"] / out["train_step_eager_us"]
    out["torch_step_over_train_step_graph"] = out["torch_autograd_step_eager_us"] / out["train_step_graph_us"]
    return out


def aux_step_times(cell, inp, T_neg=3):
    """The graph-replayed train step without and with the auxiliary loss (loss = bce + aux_loss,
    T_neg negatives per step drawn once), and the auxiliary forward / backward launches alone, in us."""
    label = (torch.rand(B, device="cuda") < 0.3).float()
    crit = torch.nn.BCELoss()
    seq = dict(inp["sequence"])
    seq["neg_" + dien_ref.SEQ_KEY] = torch.randint(0, H.WECHAT_VOCAB["feedid"], (B, (T - 1) * T_neg), device="cuda")
    out = {"T_neg": T_neg}
    for aux in (False, True):
        torch.manual_seed(0)
        m = rankops.DIEN(None, custom_gru_type=cell, vocab_sizes=H.WECHAT_VOCAB, trainable=True,
                         use_auxiliary_loss=aux, negative_sample_number=T_neg).cuda().train()
        opt = rankops.Adam(m.parameters(), lr=1e-3, capturable=True)

        def step():
            opt.zero_grad(set_to_none=False)
            res = m(inp["dense"], inp["category"], seq, inp["target"])
            loss = crit(res[0].squeeze(), label)
            (loss + res[2] if aux else loss).backward()
            opt.step()

        step()  # allocates gradients and optimizer state
        torch.cuda.synchronize()
        out["train_step_aux_graph_us" if aux else "train_step_graph_us"] = 1e3 * graph_avg_ms(step, iters=20, grad=True)
    out["aux_over_plain"] = out["train_step_aux_graph_us"] / out["train_step_graph_us"]
    # the two auxiliary launches alone, on the states of one train forward
    with torch.no_grad():
        table = m.embeddings["feedid"].weight
        ids, lens = seq[dien_ref.SEQ_KEY], seq[f"{dien_ref.SEQ_KEY}_length"]
        _, hs = rankops.dien_interest_gather(table[inp["target"]["feedid"]], table, ids, lens, m.interest_weights(),
                                             cell, return_states=True)
        neg = seq["neg_" + dien_ref.SEQ_KEY]
        per, mean = torch.empty(B, device="cuda"), torch.empty(1, device="cuda")
        one = torch.ones(1, device="cuda")
        w_aux = m.aux_project_matrix.detach()
        out["aux_forward_us"] = 1e3 * bench.graph_kernel_avg_ms(
            lambda: ops.dien_aux_loss(hs, table, ids, None, neg, lens, T, T_neg, 16, 8, w_aux, per, mean, B, hs.device))
        out["aux_backward_us"] = 1e3 * bench.graph_kernel_avg_ms(
            lambda: ops.dien_aux_loss_backward(hs, table, ids, None, neg, lens, T, T_neg, 16, 8, w_aux, one, B,
                                               hs.device))
    return out


def main():
    assert torch.cuda.is_available(), "dien_time needs a ROCm GPU"
    rankops.load_library()
    result = {"B": B, "T": T, "H": 16, "nh": 8, "device": torch.cuda.get_device_name(0),
              "max_clock_khz": getattr(torch.cuda.get_device_properties(0), "clock_rate", None),
              "sclk_before": shader_clock()}
    inp = H.to_device(H.din_inputs(B, T, H.WECHAT_VOCAB, seed=1), "cuda")
    if "--aux" in sys.argv[1:]:  # only the auxiliary-loss leg
        for cell in ("AGRU", "AUGRU"):
            result[cell] = aux_step_times(cell, inp)
            print(f"{cell}: " + ", ".join(f"{k} {v:.4g}" for k, v in result[cell].items()), flush=True)
        result["sclk_after"] = shader_clock()
        assert rankops.error_flags() == 0
        print(json.dumps(result))
        return
    for cell in ("AGRU", "AUGRU"):
        torch.manual_seed(0)
        m = rankops.DIEN(None, custom_gru_type=cell, vocab_sizes=H.WECHAT_VOCAB)
        H.randomize_eval_stats(m, 1)
        m = m.cuda().eval()
        p = {k: v.detach() for k, v in m.state_dict().items()}
        args = (inp["dense"], inp["category"], inp["sequence"], inp["target"])

        def eager():
            return dien_ref.forward(p, *args, cell_type=cell, dtype=torch.float32)

        with torch.no_grad():
            prob, logit = m(*args)
            ref = eager()
            diff = (logit - ref[1]).abs().max().item()
            # the interest launch alone, bound as the module binds it
            pl = m._plan(*args)
            row = torch.empty(B, pl["width"], device="cuda")
            ops.concat_gather(pl["segs"], B, row)
            w = m.interest_weights()

            def launch():
                ops.dien_interest(_lib.fptr(row, pl["q_col"]), pl["width"], m.embeddings["feedid"].weight, pl["seq"],
                                  pl["seq_len"], T, 16, 8, ops.DIEN_CELLS[cell], w,
                                  _lib.fptr(row, pl["state_col"]), pl["width"], None, B, row.device)

            # the train forward and the backward of the recurrence alone (chain launch + its GEMMs)
            f32 = dict(device="cuda", dtype=torch.float32)
            att, hs, ss = torch.empty(B, T, **f32), torch.empty(B, T, 8, **f32), torch.empty(B, T, 8, **f32)
            drow, dkeys = torch.randn(B, pl["width"], **f32), torch.empty(B, T, 16, **f32)

            def launch_train():
                ops.dien_interest_train(_lib.fptr(row, pl["q_col"]), pl["width"], m.embeddings["feedid"].weight,
                                        pl["seq"], pl["seq_len"], T, 16, 8, ops.DIEN_CELLS[cell], w,
                                        _lib.fptr(row, pl["state_col"]), pl["width"], att, hs, ss, B, row.device)

            def launch_backward():
                ops.dien_interest_backward(_lib.fptr(row, pl["q_col"]), pl["width"], m.embeddings["feedid"].weight,
                                           pl["seq"], 0, pl["seq_len"], T, 16, 8, ops.DIEN_CELLS[cell], w, hs, ss, att,
                                           _lib.fptr(drow, pl["state_col"]), pl["width"],
                                           _lib.fptr(drow, pl["q_col"]), pl["width"], True, dkeys, B, row.device)

            launch_train()
            r = {"logit_max_abs_diff_vs_eager_fp32": diff,
                 "interest_launch_us": 1e3 * bench.graph_kernel_avg_ms(launch),
                 "interest_train_launch_us": 1e3 * bench.graph_kernel_avg_ms(launch_train),
                 "interest_backward_us": 1e3 * bench.graph_kernel_avg_ms(launch_backward),
                 "forward_graph_us": 1e3 * graph_avg_ms(lambda: m(*args)),
                 "forward_eager_call_us": 1e3 * host_avg_ms(lambda: m(*args), iters=50),
                 "torch_loop_graph_us": 1e3 * graph_avg_ms(eager, iters=5),
                 "torch_loop_eager_us": 1e3 * host_avg_ms(eager)}
        r["torch_loop_graph_over_forward_graph"] = r["torch_loop_graph_us"] / r["forward_graph_us"]
        r["torch_loop_eager_over_forward_eager"] = r["torch_loop_eager_us"] / r["forward_eager_call_us"]
        r.update(train_step_times(cell, inp))
        result[cell] = r
        print(f"{cell}: " + ", ".join(f"{k} {v:.4g}" for k, v in r.items()), flush=True)
    result["sclk_after"] = shader_clock()
    assert rankops.error_flags() == 0
    print(json.dumps(result))


if __name__ == "__main__":
    main()
