"""What the l2 term costs the headline's prepared DIN launch (bench.py DIN configs[2], batch 4096,
T 50, H 32, frozen H2): one prepared plan with the l2 term and one with l2_out == nullptr on the same
model and inputs, each captured as a graph of 20 launches and replayed with HIP events around the
replay on its stream.  The two arms alternate over nine rounds; prints every round, then the median
and the spread (max - min) of each arm and their difference.  The library is whichever librankops.so
RANKOPS_LIB points at (default: the tree's), so a parent build and a new one are compared by running
this once per library in one session.  BATCH=<n> changes the batch, OUT=<file> also writes the lines
to a file."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import torch  # noqa: E402

LAUNCHES, ROUNDS, REPLAYS = 20, 9, 10

batch = int(os.environ.get("BATCH", "4096"))
model, inp, fn, cfg, name = bench.workload("din", batch, 0)
args = (inp["dense"], inp["category"], inp["sequence"], inp["target"])
arms = {}
with torch.no_grad():
    arms["l2"] = model.prepare(*args)
    assert isinstance(arms["l2"]()[2], torch.Tensor), "the headline model computes the l2 term"
    model.mini_batch_aware_regularization = False  # the same forward with l2_out == nullptr
    arms["no_l2"] = model.prepare(*args)
    assert not isinstance(arms["no_l2"]()[2], torch.Tensor)
torch.cuda.synchronize()

stream = torch.cuda.Stream()
graphs = {}
with torch.cuda.stream(stream):
    for k, run in arms.items():
        for _ in range(3):
            run.plan.launch_on(stream.cuda_stream)
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(LAUNCHES):
                run.plan.launch_on(stream.cuda_stream)
        g.replay()
        stream.synchronize()
        graphs[k] = g


def time_us(g):
    """Microseconds per launch over REPLAYS replays of the captured graph."""
    with torch.cuda.stream(stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g.replay()
        e0.record(stream)
        for _ in range(REPLAYS):
            g.replay()
        e1.record(stream)
        e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (REPLAYS * LAUNCHES)


for k in arms:  # untimed: the clocks settle (the first timed round used to read 1-3 us high)
    time_us(graphs[k])
    time_us(graphs[k])
lines = []
res = {k: [] for k in arms}
for r in range(ROUNDS):
    for k in arms:
        us = time_us(graphs[k])
        res[k].append(us)
        lines.append(f"round {r} {k:7s} {us:7.3f} us/launch")
med = {k: float(np.median(v)) for k, v in res.items()}
spread = {k: float(np.max(v) - np.min(v)) for k, v in res.items()}
d = med["l2"] - med["no_l2"]
lines.append(f"median l2 {med['l2']:.3f} us, no_l2 {med['no_l2']:.3f} us, difference {d:.3f} us = "
             f"{100 * d / med['l2']:.2f} % (spread l2 {spread['l2']:.3f}, no_l2 {spread['no_l2']:.3f})")
lines.append(f"library {os.path.basename(os.environ.get('RANKOPS_LIB', 'librankops.so'))}, batch {batch}")
print("\n".join(lines))
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as f:
        f.write("\n".join(lines) + "\n")
