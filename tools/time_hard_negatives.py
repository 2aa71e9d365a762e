"""Cost of hard-negative mining (num_hard_negatives = K) in the in-batch loss
against the plain entries of the same build, at the C3 step's loss shape
(B x E tower outputs, logQ on, default bf16 arithmetic), K in {16, 256, 4096}:

  select   tt_inbatch_hard_threshold: its own preparation of q and c (the two
           launches every rows entry starts with), then the selection kernel
  rows     tt_inbatch_xent_rows_hard against tt_inbatch_xent_rows
  cols     tt_inbatch_xent_cols_hard against tt_inbatch_xent_cols
  fused    tt_inbatch_softmax_xent_hard (prepare, select, rows, cols) against
           tt_inbatch_softmax_xent_loss, the default loss

Launches are replayed from one hipGraph per variant (no host time between
them), timed with device events, warm, the variants interleaved over ROUNDS
rounds; ranges printed and written to profiles/hard_negatives_cost.txt (the
DESIGN table's source).  Usage: time_hard_negatives.py [--out PATH] [--x3]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from pkg.modelling import hip_ops  # noqa: E402

B = 16384
KS = (16, 256, 4096)
REPS, ROUNDS = 10, 7
dev = torch.device("cuda:0")
OUT = os.path.join(ROOT, "profiles", "hard_negatives_cost.txt")
_lines = []


def say(line: str) -> None:
    print(line, flush=True)
    _lines.append(line)


def interleaved(variants: dict, rounds: int = ROUNDS) -> dict:
    for fn in variants.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / REPS)
    return ms


def graphed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with hip_ops.capture_guard(), torch.cuda.graph(graph, stream=side):
            for _ in range(REPS):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def show(ms: dict) -> None:
    for name, v in ms.items():
        say(f"  {name}: {min(v) * 1e3:.1f}-{max(v) * 1e3:.1f} us per call (median {float(np.median(v)) * 1e3:.1f})")


def ratio(ms: dict, a: str, b: str) -> float:
    r = [x / y for x, y in zip(ms[a], ms[b])]
    say(f"  [{a}] / [{b}]: {min(r):.2f}-{max(r):.2f}x (same-round pairs, median {float(np.median(r)):.2f}x)")
    return float(np.median(r))


def main(x3: bool) -> None:
    E = bench.main_schema().model_config.joint_embedding_size
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.relu(torch.randn(B, E, device=dev, generator=g))
    c = torch.relu(torch.randn(B, E, device=dev, generator=g))
    logq = torch.log(torch.rand(B, device=dev, generator=g) * 1e-3 + 1e-6)
    lse, rl, _ = hip_ops.inbatch_rows(q, c, logq, x3=x3)
    say(f"in-batch loss, B = {B}, E = {E}, logQ on, {'x3' if x3 else 'default (bf16)'} arithmetic; "
        f"{REPS} calls per graph replay, {ROUNDS} interleaved rounds")
    for k in KS:
        thr = hip_ops.inbatch_hard_threshold(q, c, logq, k, x3=x3)
        kept = float((thr > float("-inf")).float().mean())
        calls = {
            "select (prep + selection kernel)": lambda: hip_ops.inbatch_hard_threshold(q, c, logq, k, x3=x3),
            "rows plain": lambda: hip_ops.inbatch_rows(q, c, logq, x3=x3),
            "rows hard": lambda: hip_ops.inbatch_rows(q, c, logq, x3=x3, thr=thr),
            "cols plain": lambda: hip_ops.inbatch_cols(q, lse, c, logq, row_loss=rl, x3=x3),
            "cols hard": lambda: hip_ops.inbatch_cols(q, lse, c, logq, row_loss=rl, x3=x3, thr=thr),
            "fused plain (the default loss)": lambda: hip_ops.inbatch_fused(q, c, logq, loss_scale=1.0, x3=x3),
            "fused hard": lambda: hip_ops.inbatch_fused(q, c, logq, loss_scale=1.0, x3=x3, hard_k=k),
        }
        graphs = {name: graphed(fn) for name, fn in calls.items()}
        ms = interleaved({name: gr.replay for name, gr in graphs.items()})
        say(f"K = {k} ({kept:.0%} of the rows with a finite threshold):")
        show(ms)
        names = list(calls)
        ratio(ms, names[2], names[1])
        ratio(ms, names[4], names[3])
        ratio(ms, names[0], names[5])
        ratio(ms, names[6], names[5])


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
