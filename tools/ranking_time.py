"""Per-request ranking after DIEN scoring: device times of the segmented top-K and the grouped AUC.

Top-K, k 10, at B 32,768 with 128 candidates per request and at B 4,096 with 16 (the candidates of
a request contiguous, as a ranking stage hands them over):
  (a) topk_segments on the segment kernel (one launch, a wave per request)
  (b) topk_segments on the sort path, and topk_per_request on the same candidates (request_index
      = b // N): key kernel + radix sort + write kernel
  (c) torch.topk on the [R, N] view — the case most favourable to torch: no ragged batch has it
  (d) DIEN.score on B candidates (rk_concat_gather + rk_dien_evolve + the tail), the scoring the
      top-K follows
Routing: the segment kernel against the sort path at k 64 and at longer segments (512 .. 32,768
rows per request at B 32,768), where rankops.ranking's rule between the two is decided.
Grouped AUC at 3,000,000 rows over 100,000 groups: grouped_auc beside roc_auc (rk_auc, the ungrouped
yardstick) on the same rows, and the host loop it replaces (the copy to the host, then one
oracle.metrics.roc_auc per group; sklearn's roc_auc_score is timed on the first 2,000 groups and
scaled).

Device times are HIP events around hipGraph replays of back-to-back launches
(bench.graph_kernel_avg_ms), workspace allocation included as a caller pays it; every figure is
measured twice, the legs alternating, and both rounds are printed.  Results are compared before
timing: (a) and (b) bit for bit, (c) by value, the grouped AUC with the host loop.  The shader
clock the driver reports is printed beside the times.  Needs a GPU; prints one JSON line at the end."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (sets sys.path for rankops and tests/)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import helpers as H  # noqa: E402
import rankops  # noqa: E402
from dien_time import shader_clock  # noqa: E402
from oracle import metrics as oracle_metrics  # noqa: E402

K = 10
TOPK_SHAPES = ((32768, 128), (4096, 16))
ROUTING_SHAPES = ((32768, 128, 64), (4096, 16, 64), (32768, 512, 10), (32768, 2048, 10), (32768, 2048, 64),
                  (32768, 8192, 10), (32768, 32768, 10), (32768, 32768, 64), (262144, 128, 10))
AUC_ROWS, AUC_GROUPS = 3_000_000, 100_000
T = 50


def two_rounds(legs, **kw):
    rounds = [{name: 1e3 * bench.graph_kernel_avg_ms(fn, **kw) for name, fn in legs} for _ in range(2)]
    r = {"rounds": rounds}
    for name, _ in legs:
        r[name] = sum(x[name] for x in rounds) / len(rounds)
    return r


def topk_times(B, N, model):
    R = B // N
    gen = torch.Generator(device="cuda").manual_seed(B)
    scores = torch.randn(B, generator=gen, device="cuda")
    offsets = torch.arange(R + 1, device="cuda") * N
    req = torch.arange(B, device="cuda") // N
    seg = rankops.topk_segments(scores, offsets, K, method="segment")
    srt = rankops.topk_segments(scores, offsets, K, method="sort")
    anyo = rankops.topk_per_request(scores, req, R, K)
    ref = torch.topk(scores.view(R, N), K, dim=1)
    torch.cuda.synchronize()
    for a, b, c in zip(seg, srt, anyo):
        assert torch.equal(a, b) and torch.equal(a, c), "segment kernel and sort path must agree bit for bit"
    assert torch.equal(seg.values, ref.values), "top-K values differ from torch.topk"

    inp = H.to_device(H.din_inputs(B, T, H.WECHAT_VOCAB, seed=3), "cuda")
    hist = H.to_device(H.din_inputs(R, T, H.WECHAT_VOCAB, seed=4)["sequence"], "cuda")
    interests = model.extract_interests(hist)
    legs = (("topk_segments_kernel_us", lambda: rankops.topk_segments(scores, offsets, K, method="segment")),
            ("topk_segments_sort_us", lambda: rankops.topk_segments(scores, offsets, K, method="sort")),
            ("topk_per_request_us", lambda: rankops.topk_per_request(scores, req, R, K)),
            ("torch_topk_us", lambda: torch.topk(scores.view(R, N), K, dim=1)),
            ("dien_score_us", lambda: model.score(inp["dense"], inp["category"], inp["target"], interests, req)))
    r = two_rounds(legs)
    r.update(B=B, N=N, R=R, k=K)
    return r


def routing_times(B, N, k):
    """The segment kernel against the sort path where the routing rule has to be decided: longer
    segments (a request is one wave's serial work) and the largest k of the kernel's envelope."""
    R = B // N
    gen = torch.Generator(device="cuda").manual_seed(B + N)
    scores = torch.randn(B, generator=gen, device="cuda")
    offsets = torch.arange(R + 1, device="cuda") * N
    seg = rankops.topk_segments(scores, offsets, k, method="segment")
    srt = rankops.topk_segments(scores, offsets, k, method="sort")
    torch.cuda.synchronize()
    for a, b in zip(seg, srt):
        assert torch.equal(a, b), "segment kernel and sort path must agree bit for bit"
    r = two_rounds((("topk_segments_kernel_us", lambda: rankops.topk_segments(scores, offsets, k, method="segment")),
                    ("topk_segments_sort_us", lambda: rankops.topk_segments(scores, offsets, k, method="sort"))))
    r.update(B=B, N=N, R=R, k=k)
    return r


def auc_times():
    rng = np.random.default_rng(7)
    g = rng.integers(0, AUC_GROUPS, AUC_ROWS).astype(np.int64)
    s = rng.random(AUC_ROWS).astype(np.float32)
    y = (rng.random(AUC_ROWS) < 0.3).astype(np.float32)
    d_s, d_y, d_g = (torch.from_numpy(a).cuda() for a in (s, y, g))
    got, table = rankops.grouped_auc(d_s, d_y, d_g, return_groups=True)

    t0 = time.perf_counter()
    h_s, h_y, h_g = d_s.cpu().numpy(), d_y.cpu().numpy(), d_g.cpu().numpy()
    order = np.argsort(h_g, kind="stable")
    h_s, h_y, h_g = h_s[order], h_y[order], h_g[order]
    starts = np.flatnonzero(np.r_[True, h_g[1:] != h_g[:-1]])
    ends = np.r_[starts[1:], len(h_g)]
    num = rows = 0.0
    for a, b in zip(starts, ends):
        auc = oracle_metrics.roc_auc(h_s[a:b], h_y[a:b])
        if auc == auc:
            num += (b - a) * auc
            rows += b - a
    host_loop_s = time.perf_counter() - t0
    assert abs(float(got.gauc) - num / rows) < 1e-12 and int(got.valid_rows) == rows, (float(got.gauc), num / rows)

    from sklearn.metrics import roc_auc_score
    sample = 2000
    t0 = time.perf_counter()
    for a, b in zip(starts[:sample], ends[:sample]):
        if 0 < h_y[a:b].sum() < b - a:
            roc_auc_score(h_y[a:b], h_s[a:b])
    sklearn_s = (time.perf_counter() - t0) * len(starts) / sample

    legs = (("grouped_auc_us", lambda: rankops.grouped_auc(d_s, d_y, d_g)),
            ("roc_auc_us", lambda: rankops.roc_auc(d_s, d_y)))
    r = two_rounds(legs, per_graph=2, iters=5)
    r.update(rows=AUC_ROWS, groups=int(len(starts)), gauc=float(got.gauc), host_loop_s=host_loop_s,
             sklearn_loop_s_scaled_from_2000_groups=sklearn_s)
    return r


def main():
    assert torch.cuda.is_available(), "ranking_time needs a ROCm GPU"
    rankops.load_library()
    result = {"device": torch.cuda.get_device_name(0),
              "max_clock_khz": getattr(torch.cuda.get_device_properties(0), "clock_rate", None),
              "sclk_before": shader_clock(), "topk": []}
    torch.manual_seed(0)
    model = rankops.DIEN(None, custom_gru_type="AUGRU", vocab_sizes=H.WECHAT_VOCAB).cuda().eval()
    for B, N in TOPK_SHAPES:
        r = topk_times(B, N, model)
        result["topk"].append(r)
        print(f"top-{K} B {B} N {N}: " + ", ".join(f"{k} {v:.4g}" for k, v in r.items() if isinstance(v, float)),
              flush=True)
        print(f"  rounds {r['rounds']}", flush=True)
    result["routing"] = []
    for B, N, k in ROUTING_SHAPES:
        r = routing_times(B, N, k)
        result["routing"].append(r)
        print(f"routing B {B} N {N} k {k}: kernel {r['topk_segments_kernel_us']:.4g} us, sort "
              f"{r['topk_segments_sort_us']:.4g} us, rounds {r['rounds']}", flush=True)
    result["grouped_auc"] = r = auc_times()
    print("grouped AUC: " + ", ".join(f"{k} {v:.5g}" for k, v in r.items() if isinstance(v, float)), flush=True)
    print(f"  rounds {r['rounds']}", flush=True)
    result["sclk_after"] = shader_clock()
    assert rankops.error_flags() == 0
    print(json.dumps(result))


if __name__ == "__main__":
    main()
