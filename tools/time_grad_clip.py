"""Cost of gradient clipping (clipvalue / clipnorm / global_clipnorm) at the
C3 train step (bench.py's model and batches, B = 16384, Adagrad).

  step     the graphed step: the default one; the unclipped step on the path a
           clipping optimizer forces (no update from inside the backward; the
           difference is the price of leaving the fused dense apply); each of
           clipvalue, clipnorm and global_clipnorm on top of it, with settings
           that trigger (every region is read and written).
  kernels  the launches alone over the step's own gradients: the norm pass
           (tt_grad_sumsq: partial sums, then the per-variable reduction) and
           the apply (tt_grad_clip_apply) as a clamp and as a scale, with the
           bytes they move against the HBM peak, and the launch counts.

Launches are replayed from one hipGraph per variant (no host time between
them), timed with device events, warm, the variants interleaved over ROUNDS
rounds; ranges printed and written to profiles/grad_clip_cost.txt (the DESIGN
table's source).  Usage: time_grad_clip.py [step kernels] [--out PATH]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from pkg import _native  # noqa: E402
from pkg.modelling import hip_ops  # noqa: E402
from pkg.modelling.models import two_tower_model as ttm  # noqa: E402
from pkg.modelling.optimizer_factory import OptimizerFactory  # noqa: E402

B = 16384
REPS, ROUNDS = 20, 7
HBM_PEAK = 8.0e12  # bytes/s, MI355X
dev = torch.device("cuda:0")
OUT = os.path.join(ROOT, "profiles", "grad_clip_cost.txt")
_lines = []


def say(line: str) -> None:
    print(line, flush=True)
    _lines.append(line)


def interleaved(variants: dict, reps: int, rounds: int = ROUNDS) -> dict:
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / reps)
    return ms


def graphed(fn, reps: int):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with hip_ops.capture_guard(), torch.cuda.graph(graph, stream=side):
            for _ in range(reps):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def show(ms: dict) -> None:
    for name, v in ms.items():
        say(f"  {name}: {min(v) * 1e3:.1f}-{max(v) * 1e3:.1f} us per call (median {float(np.median(v)) * 1e3:.1f})")


def diff(ms: dict, a: str, b: str) -> None:
    d = [x - y for x, y in zip(ms[a], ms[b])]
    say(f"  [{a}] - [{b}]: {min(d) * 1e3:.1f}-{max(d) * 1e3:.1f} us (same-round pairs, "
        f"median {float(np.median(d)) * 1e3:.1f})")


def c3_model(data, **clip):
    schema = bench.main_schema()
    schema.set_candidate_prob_lookup(data.prob_lookup())
    mc = schema.model_config
    m = ttm.TwoTowerModel(list(schema.query_features), list(schema.candidate_features), "article_id",
                          mc.joint_embedding_size, mc.query_tower_units, mc.candidate_tower_units,
                          candidate_prob_lookup=schema.training_config.candidate_prob_lookup, device=dev, seed=0)
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", dict({"learning_rate": 0.05}, **clip)))
    return m


VARIANTS = [("default step", None, {}), ("unclipped, no update inside the backward", False, {}),
            ("clipvalue=1e-4", None, {"clipvalue": 1e-4}), ("clipnorm=1e-3", None, {"clipnorm": 1e-3}),
            ("global_clipnorm=1e-2", None, {"global_clipnorm": 1e-2})]


def step() -> None:
    data = bench.SyntheticHM(dev, seed=1234)
    pool = [data.batch(B) for _ in range(4)]
    steps = {}
    for name, dense_early, clip in VARIANTS:
        m = c3_model(data, **clip)
        was = ttm.DENSE_EARLY
        if dense_early is not None:
            ttm.DENSE_EARLY = dense_early  # read while the step is issued: the capture holds the choice
        try:
            g = ttm.GraphedTrainStep(m, pool[0], warmup=2)
        finally:
            ttm.DENSE_EARLY = was
        steps[name] = (g, [g.pack(b) for b in pool], [0])

    def run(name):
        g, packed, i = steps[name]
        g(packed=packed[i[0] % len(packed)])
        i[0] += 1

    ms = interleaved({k: (lambda k=k: run(k)) for k in steps}, reps=100)
    say(f"graphed C3 train step, B = {B}, Adagrad:")
    show(ms)
    names = list(steps)
    diff(ms, names[1], names[0])
    for n in names[2:]:
        diff(ms, n, names[1])
    for name, (g, _, _) in steps.items():
        opt = g.model.optimizer
        opt.check_status(dev)
        f = opt.last_clip_factors
        say(f"  {name}: loss after the timed steps {float(g.out['loss'].item()):.4f}"
            + (f", factors {float(f.min()):.3e} .. {float(f.max()):.3e}" if f is not None else ""))


def kernels() -> None:
    data = bench.SyntheticHM(dev, seed=1234)
    m = c3_model(data, global_clipnorm=1.0)
    m.train_step(data.batch(B))  # leaves this step's gradients in place
    opt = m.optimizer
    names, regions = opt._clip_regions(m.towers)
    nv, nbytes = len(names), sum(g.numel() for g, _, _ in regions) * 4
    chunks = -(-len(regions) // _native.MAX_CLIP_REGIONS)
    say(f"C3 gradients, B = {B}: {len(regions)} regions of {nv} variables, {nbytes / 1e6:.1f} MB of values; "
        f"launches per step: norm pass {2 * chunks}, apply {chunks}")
    arr = hip_ops.clip_regions(regions, nv)
    sumsq = torch.zeros(nv, dtype=torch.float64, device=dev)
    factor = torch.ones(nv, dtype=torch.float32, device=dev)
    hip_ops.grad_sumsq(arr, nv, None, sumsq)
    # a norm one ulp above the bound: the apply reads and writes every value and barely moves it
    near = torch.full((nv,), 1.0000002, dtype=torch.float64, device=dev)
    calls = {
        "norm pass (tt_grad_sumsq)": (lambda: hip_ops.grad_sumsq(arr, nv, None, sumsq), nbytes),
        "apply, scale (clipnorm)": (lambda: hip_ops.grad_clip_apply(arr, nv, None, 1.0, None, near, factor),
                                    2 * nbytes),
        "apply, clamp (clipvalue)": (lambda: hip_ops.grad_clip_apply(arr, nv, 1e-4, None, None, None, factor),
                                     2 * nbytes),
        "apply, factor 1 (nothing read)": (lambda: hip_ops.grad_clip_apply(arr, nv, None, 1e30, None, sumsq, factor),
                                           0),
    }
    graphs = {k: graphed(fn, REPS) for k, (fn, _) in calls.items()}
    ms = {k: [t / REPS for t in v] for k, v in interleaved({k: g.replay for k, g in graphs.items()}, reps=1).items()}
    show(ms)
    for k, (_, moved) in calls.items():
        if moved:
            bw = moved / (float(np.median(ms[k])) * 1e-3)
            say(f"  {k}: {moved / 1e6:.1f} MB moved, {bw / 1e12:.2f} TB/s at the median "
                f"({100 * bw / HBM_PEAK:.0f}% of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak)")


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--out" in args:
        i = args.index("--out")
        OUT = args[i + 1]
        del args[i:i + 2]
    torch.cuda.set_device(dev)
    for part in args or ["step", "kernels"]:
        {"step": step, "kernels": kernels}[part]()
    with open(OUT, "w") as fh:
        fh.write("\n".join(_lines) + "\n")
