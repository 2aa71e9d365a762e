"""Cost of the set-valued ranking metrics (tt_rank_metrics) next to what they
sit beside: tt_recall_hits on the same lists and ks (the recall-only yardstick),
the plain search that produced the lists, and the host alternative the kernel
replaces (a device-to-host copy of the lists plus the package's numpy path,
pkg.modelling.metrics.ranking_metrics.host_rank_metrics).

Points: lists of 2048 x 100 and 131,072 x 100 (k = 100 over 105,542 candidates
x 128 as bench.py's index), ks = 1 / 12 / 100, truth T = 1 and T = 12 with
about 10 % of the queries empty.  tt_rank_metrics is timed with accumulators
(both launches: the per-query kernel and the deterministic reduction) and
without (the first launch alone).  Device events around REPS back-to-back
calls, warm, the variants of a point interleaved over ROUNDS rounds; prints
each variant's median and range and its same-round ratio to tt_recall_hits.
The host path is wall-clock (it is host work) over fewer rounds.
--out FILE also writes the lines there."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pkg.modelling import hip_ops  # noqa: E402
from pkg.modelling.indices.brute_force import BruteForceIndex  # noqa: E402
from pkg.modelling.metrics.ranking_metrics import host_rank_metrics  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--chunk", type=int, default=131072)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--host-rounds-large", type=int, default=1)
args = ap.parse_args()

N, E, K = 105542, 128, 100
KS = [1, 12, 100]
dev = torch.device("cuda:0")
g = torch.Generator(device=dev)
g.manual_seed(0)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure(point, variants, reps, rounds, base):
    for fn in variants.values():  # warm: tables, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            ms[name].append(timed(fn, reps[name] if isinstance(reps, dict) else reps))
    for name, v in ms.items():
        ratio = [x / p for x, p in zip(v, ms[base])]
        say(f"{point} | {name}: median {float(np.median(v)) * 1e3:.1f} us, range {min(v) * 1e3:.1f}-"
            f"{max(v) * 1e3:.1f}; / {base} median {float(np.median(ratio)):.2f}, range {min(ratio):.2f}-"
            f"{max(ratio):.2f}")


def truth_for(lists, T):
    """[Q, T] int32: about 10 % of the rows empty; the others hold 1..T ids, half of them from the row's own list."""
    Q = lists.shape[0]
    own = torch.gather(lists, 1, torch.randint(0, K, (Q, T), generator=g, device=dev))
    other = torch.randint(0, N, (Q, T), generator=g, device=dev, dtype=torch.int32)
    t = torch.where(torch.rand(Q, T, generator=g, device=dev) < 0.5, own, other)
    count = torch.randint(1, T + 1, (Q, 1), generator=g, device=dev)
    count[torch.rand(Q, 1, generator=g, device=dev) < 0.1] = 0
    t[torch.arange(T, device=dev).reshape(1, -1) >= count] = -1
    return t.contiguous()


def acc_tensors():
    return (torch.zeros(len(KS), 4, dtype=torch.float64, device=dev),
            torch.zeros(len(KS), 2, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))


cand = torch.randn(N, E, generator=g, device=dev) * 0.3
index = BruteForceIndex(K, None, [(torch.arange(N, dtype=torch.int32), cand)], device=dev)
say(f"index {N} x {E}, k = {K}, ks = {KS}; {torch.cuda.get_device_name(0)}")

for Q, reps, search_reps, host_rounds in ((2048, 50, 10, 3), (args.chunk, 10, 2, args.host_rounds_large)):
    q = torch.randn(Q, E, generator=g, device=dev) * 0.3
    _, lists = index.search(q)
    hits64 = torch.zeros(len(KS), dtype=torch.int64, device=dev)
    for T in (1, 12):
        truth = truth_for(lists, T)
        acc = acc_tensors()
        vals, hits, m = hip_ops.rank_metrics(lists, truth, KS, acc)
        empty = float((m == 0).float().mean())
        # the device answer is the host path's on a sample
        hv, hh, hm = host_rank_metrics(lists[:512].cpu().numpy(), truth[:512].cpu().numpy(), KS)
        assert np.array_equal(vals[:512].cpu().numpy().view(np.int32), hv.view(np.int32))
        assert np.array_equal(hits[:512].cpu().numpy(), hh) and np.array_equal(m[:512].cpu().numpy(), hm)
        first_true = truth[:, 0].contiguous()
        variants = {
            "tt_recall_hits": lambda: hip_ops.recall_hits(first_true, lists, KS, hits64),
            "tt_rank_metrics, both launches": lambda: hip_ops.rank_metrics(lists, truth, KS, acc),
            "tt_rank_metrics, per-query launch alone": lambda: hip_ops.rank_metrics(lists, truth, KS),
            "plain search k=100": lambda: index.search(q),
        }
        per = {name: reps for name in variants}
        per["plain search k=100"] = search_reps
        point = f"{Q} x {K} lists, T = {T} ({empty:.1%} empty)"
        measure(point, variants, per, args.rounds, "tt_recall_hits")
        wall = []
        for _ in range(host_rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_rank_metrics(lists.cpu().numpy(), truth.cpu().numpy(), KS)
            wall.append(time.perf_counter() - t0)
        say(f"{point} | host: D2H copy + numpy path: median {float(np.median(wall)) * 1e3:.1f} ms over "
            f"{host_rounds} run(s), range {min(wall) * 1e3:.1f}-{max(wall) * 1e3:.1f}")
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
