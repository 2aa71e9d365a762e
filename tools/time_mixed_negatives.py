"""Cost of mixed negative sampling (num_sampled_negatives = M) in the in-batch
loss against the plain fused loss of the same build, at the C3 step's loss
shape (B x E tower outputs, logQ on, default bf16 arithmetic), M in
{1024, 4096, 16384}:

  fused mixed  tt_inbatch_softmax_xent_mixed (q [B] against c [B + M]: prepare,
               rows, cols) against tt_inbatch_softmax_xent_loss at n = B, the
               default loss; the ratio is printed beside (B + M) / B, what the
               wider score matrix alone would cost
  sampler      tt_mixed_candidates alone: 3 columns, a catalogue of the
               105,542 H&M articles

Launches are replayed from one hipGraph per variant (no host time between
them), timed with device events, warm, the variants interleaved over ROUNDS
rounds; ranges printed and written to profiles/mixed_negatives_cost.txt.
Usage: time_mixed_negatives.py [--out PATH] [--x3]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from pkg.modelling import hip_ops  # noqa: E402
from time_hard_negatives import REPS, ROUNDS, graphed, interleaved  # noqa: E402

B = 16384
MS = (1024, 4096, 16384)
N_CAT = 105542
dev = torch.device("cuda:0")
OUT = os.path.join(ROOT, "profiles", "mixed_negatives_cost.txt")
_lines = []


def say(line: str) -> None:
    print(line, flush=True)
    _lines.append(line)


def main(x3: bool) -> None:
    E = bench.main_schema().model_config.joint_embedding_size
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.relu(torch.randn(B, E, device=dev, generator=g))
    call = torch.relu(torch.randn(B + max(MS), E, device=dev, generator=g))
    lall = torch.log(torch.rand(B + max(MS), device=dev, generator=g) * 1e-3 + 1e-6)
    cat = torch.randint(0, N_CAT, (3, N_CAT), device=dev, dtype=torch.int32, generator=g)
    cols = [torch.randint(0, N_CAT, (B,), device=dev, dtype=torch.int32, generator=g) for _ in range(3)]
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    say(f"in-batch loss, B = {B}, E = {E}, logQ on, {'x3' if x3 else 'default (bf16)'} arithmetic; "
        f"{REPS} calls per graph replay, {ROUNDS} interleaved rounds")
    for m in MS:
        c, logq = call[:B + m].contiguous(), lall[:B + m].contiguous()
        c0, logq0 = call[:B].contiguous(), lall[:B].contiguous()
        out = torch.empty(3, B + m, dtype=torch.int32, device=dev)
        calls = {
            "fused plain (the default loss, n = B)": lambda: hip_ops.inbatch_fused(q, c0, logq0, loss_scale=1.0, x3=x3),
            "fused mixed": lambda: hip_ops.inbatch_fused_mixed(q, c, logq, loss_scale=1.0, x3=x3),
            "sampler (tt_mixed_candidates, 3 columns)": lambda: hip_ops.mixed_candidates(cols, cat, m, 0, step, out),
        }
        graphs = {name: graphed(fn) for name, fn in calls.items()}
        ms = interleaved({name: gr.replay for name, gr in graphs.items()})
        say(f"M = {m}:")
        for name, v in ms.items():
            say(f"  {name}: {min(v) * 1e3:.1f}-{max(v) * 1e3:.1f} us per call (median {float(np.median(v)) * 1e3:.1f})")
        names = list(calls)
        r = [x / y for x, y in zip(ms[names[1]], ms[names[0]])]
        say(f"  [{names[1]}] / [{names[0]}]: {min(r):.2f}-{max(r):.2f}x (same-round pairs, median "
            f"{float(np.median(r)):.2f}x); (B + M) / B = {(B + m) / B:.2f}")


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--out" in args:
        i = args.index("--out")
        OUT = args[i + 1]
        del args[i:i + 2]
    torch.cuda.set_device(dev)
    main("--x3" in args)
    with open(OUT, "w") as fh:
        fh.write("\n".join(_lines) + "\n")
