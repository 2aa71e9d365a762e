"""Cost of per-example sample weights ("__weight__" in the batch) against the
unweighted step of the same build.

  step   the graphed C3 train step (bench.py's model and batches) with a weight
         column against the same step without it.  The weighted step runs the
         rows entry, tt_inbatch_weight_rows, the cols entry and tt_sum where
         the unweighted one runs the fused entry.
  loss   where the difference goes, at the step's loss shape (B x E tower
         outputs, logQ on): the fused entry; rows + cols + tt_sum (each entry
         with its own preparation of q and c); the same with the fold between
         them; the fold alone; tt_sum alone.

Launches are replayed from one hipGraph per variant (no host time between
them), timed with device events, warm, the variants interleaved over ROUNDS
rounds; ranges printed and written to profiles/weight_cost.txt (the DESIGN
table's source).  Usage: time_weight.py [step loss] [--out PATH]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from pkg.modelling import hip_ops  # noqa: E402
from pkg.modelling.models.two_tower_model import WEIGHT_KEY, GraphedTrainStep, TwoTowerModel  # noqa: E402
from pkg.modelling.optimizer_factory import OptimizerFactory  # noqa: E402

B = 16384
REPS, ROUNDS = 20, 7
dev = torch.device("cuda:0")
OUT = os.path.join(ROOT, "profiles", "weight_cost.txt")
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


def c3_model(data):
    schema = bench.main_schema()
    schema.set_candidate_prob_lookup(data.prob_lookup())
    mc = schema.model_config
    m = TwoTowerModel(list(schema.query_features), list(schema.candidate_features), "article_id",
                      mc.joint_embedding_size, mc.query_tower_units, mc.candidate_tower_units,
                      candidate_prob_lookup=schema.training_config.candidate_prob_lookup, device=dev, seed=0)
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", {"learning_rate": 0.05}))
    return m


def weights(rng) -> torch.Tensor:
    """Time-decay weights: exp(-age / 90 days) over two years, the newest at 1."""
    w = np.exp(-rng.uniform(0, 730, B) / 90.0).astype(np.float32)
    w[0] = 1.0
    return torch.as_tensor(w, device=dev)


def step() -> None:
    data = bench.SyntheticHM(dev, seed=1234)
    rng = np.random.default_rng(5)
    pool = [data.batch(B) for _ in range(4)]
    steps = {}
    for name, weighted in (("unweighted", False), ("with __weight__", True)):
        batches = [dict(b, **{WEIGHT_KEY: weights(rng)}) for b in pool] if weighted else pool
        m = c3_model(data)
        m.sample_weight_scale = 3.0
        g = GraphedTrainStep(m, batches[0], warmup=2)
        steps[name] = (g, [g.pack(b) for b in batches], [0])

    def run(name):
        g, packed, i = steps[name]
        g(packed=packed[i[0] % len(packed)])
        i[0] += 1

    ms = interleaved({k: (lambda k=k: run(k)) for k in steps}, reps=100)
    say(f"graphed C3 train step, B = {B}:")
    show(ms)
    names = list(steps)
    diff(ms, names[1], names[0])
    for name, (g, _, _) in steps.items():
        g.model.optimizer.check_status(dev)
        say(f"  {name}: loss after the timed steps {float(g.out['loss'].item()):.4f}")


def loss() -> None:
    E = bench.main_schema().model_config.joint_embedding_size
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.relu(torch.randn(B, E, device=dev, generator=g))
    c = torch.relu(torch.randn(B, E, device=dev, generator=g))
    logq = torch.log(torch.rand(B, device=dev, generator=g) * 1e-3 + 1e-6)
    w = weights(np.random.default_rng(1))
    lse, rl, dq = hip_ops.inbatch_rows(q, c, logq)

    def chain(fold: bool):
        lse, rl, dq = hip_ops.inbatch_rows(q, c, logq)
        if fold:
            lse, rl, wl = hip_ops.inbatch_weight_rows(w, lse, rl, dq)
        hip_ops.inbatch_cols(q, lse, c, logq, row_loss=rl)
        hip_ops.loss_sum(wl if fold else rl)

    calls = {
        "fused entry (loss inside)": lambda: hip_ops.inbatch_fused(q, c, logq, loss_scale=1.0),
        "rows + cols + tt_sum": lambda: chain(False),
        "rows + fold + cols + tt_sum": lambda: chain(True),
        "fold alone (tt_inbatch_weight_rows)": lambda: hip_ops.inbatch_weight_rows(w, lse, rl, dq),
        "fold alone, no dq (evaluation)": lambda: hip_ops.inbatch_weight_rows(w, lse, rl),
        "tt_sum alone": lambda: hip_ops.loss_sum(rl),
    }
    graphs = {k: graphed(fn, REPS) for k, fn in calls.items()}
    ms = {k: [t / REPS for t in v] for k, v in interleaved({k: gr.replay for k, gr in graphs.items()}, reps=1).items()}
    say(f"in-batch loss, B = {B}, E = {E}, logQ on, default (bf16) arithmetic:")
    show(ms)
    names = list(calls)
    diff(ms, names[1], names[0])
    diff(ms, names[2], names[1])
    med = float(np.median(ms[names[3]]))
    say(f"  fold alone: {2 * B * E * 4 / med / 1e9:.2f} TB/s of dq traffic (read + write) at the median")


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--out" in args:
        i = args.index("--out")
        OUT = args[i + 1]
        del args[i:i + 2]
    torch.cuda.set_device(dev)
    for part in args or ["step", "loss"]:
        {"step": step, "loss": loss}[part]()
    with open(OUT, "w") as fh:
        fh.write("\n".join(_lines) + "\n")
