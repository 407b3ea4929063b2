"""Request-level DIEN scoring against the fused kernel (T 50, H 16, nh 8, WeChat feedid vocabulary,
both cells): B candidates, N per request (R = B / N histories), at B 4096 and 32768, N 1, 16, 128.

  (a) rk_dien_interest on the history ids replicated per candidate: what a caller had before
  (b) rk_dien_extract over the R histories + rk_dien_evolve over the B candidates
  (c) rk_dien_evolve alone: the interests of the R users are cached
  and rk_dien_extract alone.

The candidates of a request are contiguous in the batch (request_index = b // N), which is how a
ranking stage would hand them over and gives (a) the same cache locality on its replicated ids.
Device times are HIP events around hipGraph replays of 20 back-to-back launches
(bench.graph_kernel_avg_ms), all in one process; every figure is measured twice, the legs
alternating, and both rounds are printed.  Before timing, (b)'s states are compared bit for bit
with (a)'s.  The shader clock the driver reports is printed beside the times.
Needs a GPU; prints one JSON line at the end."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (sets sys.path for rankops and tests/)
import torch  # noqa: E402

import helpers as H  # noqa: E402
import rankops  # noqa: E402
from dien_time import shader_clock  # noqa: E402
from rankops import ops  # noqa: E402

T, HD, NH = 50, 16, 8
BATCHES, PER_REQUEST = (4096, 32768), (1, 16, 128)


def measure(B, N, cell, w, table, gen):
    R = B // N
    dev = table.device
    f32 = dict(device=dev, dtype=torch.float32)
    ids = torch.randint(0, table.shape[0] - 1, (R, T), generator=gen, device=dev)
    lens = torch.randint(1, T + 1, (R,), generator=gen, device=dev)
    req = torch.arange(B, device=dev) // N
    query = table[torch.randint(0, table.shape[0] - 1, (B,), generator=gen, device=dev)].contiguous()
    rep_ids, rep_lens = ids[req].contiguous(), lens[req].contiguous()
    out_a, out_b, hs = torch.empty(B, NH, **f32), torch.empty(B, NH, **f32), torch.empty(R, T, NH, **f32)
    c = ops.DIEN_CELLS[cell]

    def fused():
        ops.dien_interest(query.data_ptr(), HD, table, rep_ids, rep_lens, T, HD, NH, c, w, out_a.data_ptr(), NH, None,
                          B, dev)

    def extract():
        ops.dien_extract(table, ids, lens, T, HD, NH, w[:4], hs, R, dev)

    def evolve():
        ops.dien_evolve(query.data_ptr(), HD, hs, lens, req, HD, c, w[4:], out_b.data_ptr(), NH, None, B, dev)

    def both():
        extract()
        evolve()

    fused()
    both()
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b), "extract + evolve must be bit-equal to the fused kernel"
    legs = (("fused_us", fused), ("extract_evolve_us", both), ("evolve_us", evolve), ("extract_us", extract))
    rounds = [{k: 1e3 * bench.graph_kernel_avg_ms(fn) for k, fn in legs} for _ in range(2)]
    r = {"B": B, "N": N, "R": R, "rounds": rounds}
    for k, _ in legs:
        r[k] = sum(x[k] for x in rounds) / len(rounds)
    r["fused_over_extract_evolve"] = r["fused_us"] / r["extract_evolve_us"]
    r["fused_over_evolve"] = r["fused_us"] / r["evolve_us"]
    return r


def main():
    assert torch.cuda.is_available(), "dien_requests_time needs a ROCm GPU"
    rankops.load_library()
    result = {"T": T, "H": HD, "nh": NH, "device": torch.cuda.get_device_name(0),
              "max_clock_khz": getattr(torch.cuda.get_device_properties(0), "clock_rate", None),
              "sclk_before": shader_clock(), "runs": []}
    gen = torch.Generator(device="cuda").manual_seed(1)
    for cell in ("AGRU", "AUGRU"):
        torch.manual_seed(0)
        m = rankops.DIEN(None, custom_gru_type=cell, vocab_sizes=H.WECHAT_VOCAB).cuda().eval()
        w = [x.detach() for x in m.interest_weights()]
        table = m.embeddings["feedid"].weight.detach()
        for B in BATCHES:
            for N in PER_REQUEST:
                r = measure(B, N, cell, w, table, gen)
                r["cell"] = cell
                result["runs"].append(r)
                print(f"{cell} B {B} N {N}: " + ", ".join(f"{k} {v:.4g}" for k, v in r.items()
                                                           if isinstance(v, float)), flush=True)
    result["sclk_after"] = shader_clock()
    assert rankops.error_flags() == 0
    print(json.dumps(result))


if __name__ == "__main__":
    main()
