"""Cost of a sequence feature (pooled embedding bags) against yardsticks the
project already had.

  kernels  B = 16384 bags of L = 16 ids into a 105,542 x 64 table, Zipf(1.1)
           and uniform ids:
             tt_gather_bag          against tt_gather_grouped of ONE segment with
                                    the same B * L ids of the same table (reads
                                    the same rows, writes L times more) and
                                    against a copy_ of B * L * dim * 4 bytes;
             tt_bag_grad_expand + the flat sparse Adagrad call on B * L lookups
                                    against the sparse call alone on B lookups.
  step     the graphed C3 train step (bench.py's model and batches) with one
           such query-side history feature (the customer's last 16 articles,
           mean-pooled, dim 64) against the same step without it.

Launches are replayed from one hipGraph per variant (no host time between
them), timed with device events, warm, the variants interleaved over ROUNDS
rounds; ranges printed and written to profiles/bag_cost.txt (the DESIGN
table's source).  Usage: time_bag.py [kernels step] [--out PATH]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from pkg import dtypes  # noqa: E402
from pkg.modelling import hip_ops  # noqa: E402
from pkg.modelling.models.two_tower_model import GraphedTrainStep, TwoTowerModel  # noqa: E402
from pkg.modelling.optimizer_factory import OptimizerFactory  # noqa: E402
from pkg.schema.features import Feature, FeatureFamily  # noqa: E402

B, V, DIM, L = 16384, 105542, 64, 16
REPS, ROUNDS = 20, 7
dev = torch.device("cuda:0")
OUT = os.path.join(ROOT, "profiles", "bag_cost.txt")
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


def ratio(ms: dict, a: str, b: str) -> str:
    r = [x / y for x, y in zip(ms[a], ms[b])]
    return f"  {a} / {b}: {min(r):.2f}-{max(r):.2f} (same-round pairs, median {float(np.median(r)):.2f})"


def bag_ids(rng, kind: str) -> np.ndarray:
    """[B, L] full bags of Zipf(1.1) or uniform rows."""
    if kind == "zipf":
        ids = rng.choice(V, size=(B, L), p=bench.zipf_probs(V, 1.1)).astype(np.int32)
    else:
        ids = rng.integers(0, V, (B, L)).astype(np.int32)
    return ids


def kernels() -> None:
    rng = np.random.default_rng(0)
    table = torch.empty(V, DIM, device=dev).uniform_(-0.05, 0.05)
    acc = torch.full_like(table, 0.1)
    table1, acc1 = table.clone(), acc.clone()
    out = torch.empty(B, DIM, device=dev)
    scale = torch.empty(B, device=dev)
    flat_out = torch.empty(B * L, DIM, device=dev)
    dout = torch.randn(B, DIM, device=dev)
    ids_flat = torch.empty(B * L, dtype=torch.int32, device=dev)
    G = torch.zeros(B * L, DIM, device=dev)
    src, dst = (torch.empty(B * L * DIM * 4, dtype=torch.uint8, device=dev) for _ in range(2))
    for kind in ("zipf", "uniform"):
        ids = torch.as_tensor(bag_ids(rng, kind), device=dev)
        flat = ids.reshape(-1).contiguous()
        one = flat[:B].contiguous()
        hip_ops.gather_bag([(table, ids, "mean", out, 0, scale)], B)

        def bag_update():
            hip_ops.bag_grad_expand([(V, ids, "mean", dout, 0, scale, ids_flat, G)], B)
            hip_ops.sparse_adagrad([dict(table=table, slot0=acc, ids=[ids_flat], grad_col_offset=[0], grad=G)],
                                   B * L, None, 0.05, 1e-7, ws_tag="sparse_bag")

        calls = {
            "tt_gather_bag": lambda: hip_ops.gather_bag([(table, ids, "mean", out, 0, scale)], B),
            "tt_gather_grouped, B*L ids": lambda: hip_ops.gather_grouped([(table, flat, 0)], B * L, flat_out),
            f"copy {B * L * DIM * 4 >> 20} MiB": lambda: dst.copy_(src),
            "tt_bag_grad_expand": lambda: hip_ops.bag_grad_expand(
                [(V, ids, "mean", dout, 0, scale, ids_flat, G)], B),
            "expand + flat sparse Adagrad, B*L lookups": bag_update,
            "sparse Adagrad alone, B lookups": lambda: hip_ops.sparse_adagrad(
                [dict(table=table1, slot0=acc1, ids=[one], grad_col_offset=[0])], B, dout, 0.05, 1e-7),
        }
        graphs = {k: graphed(fn, REPS) for k, fn in calls.items()}
        ms = {k: [t / REPS for t in v] for k, v in interleaved({k: g.replay for k, g in graphs.items()}, reps=1).items()}
        say(f"kernels, {kind} ids: B = {B}, L = {L}, table {V} x {DIM} fp32 "
            f"({B * L * DIM * 4 >> 20} MiB of rows read per bag launch, {B * DIM * 4 >> 20} MiB written):")
        show(ms)
        names = list(calls)
        say(ratio(ms, names[0], names[1]))
        say(ratio(ms, names[0], names[2]))
        say(ratio(ms, names[4], names[5]))
        med = float(np.median(ms[names[0]]))
        say(f"  tt_gather_bag: {B * L * DIM * 4 / med / 1e9:.2f} TB/s of row reads at the median")
        hip_ops.sparse_status(dev, "sparse_bag")
        del graphs


def c3_model(data, history: bool):
    schema = bench.main_schema()
    schema.set_candidate_prob_lookup(data.prob_lookup())
    qf, cf = list(schema.query_features), list(schema.candidate_features)
    if history:
        f = Feature("history", dtypes.string, FeatureFamily.QUERY, embedding_size=DIM, sequence_length=L,
                    pooling="mean")
        f.vocab = np.arange(V).astype(str)
        f.is_built = True
        qf.append(f)
    mc = schema.model_config
    m = TwoTowerModel(qf, cf, "article_id", mc.joint_embedding_size, mc.query_tower_units, mc.candidate_tower_units,
                      candidate_prob_lookup=schema.training_config.candidate_prob_lookup, device=dev, seed=0)
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", {"learning_rate": 0.05}))
    return m


def step() -> None:
    data = bench.SyntheticHM(dev, seed=1234)
    rng = np.random.default_rng(5)
    pool = [data.batch(B) for _ in range(4)]
    steps = {}
    for name, history in (("default", False), (f"with history L={L} dim={DIM}", True)):
        batches = pool
        if history:
            batches = []
            for b in pool:
                h = bag_ids(rng, "zipf") + 1  # table rows 1..V
                h[np.arange(L)[None, :] >= rng.integers(0, L + 1, B)[:, None]] = -1
                batches.append(dict(b, history=torch.as_tensor(h, device=dev)))
        g = GraphedTrainStep(c3_model(data, history), batches[0], warmup=2)
        steps[name] = (g, [g.pack(b) for b in batches], [0])

    def run(name):
        g, packed, i = steps[name]
        g(packed=packed[i[0] % len(packed)])
        i[0] += 1

    ms = interleaved({k: (lambda k=k: run(k)) for k in steps}, reps=100)
    say(f"graphed C3 train step, B = {B}:")
    show(ms)
    names = list(steps)
    d = [b - a for a, b in zip(ms[names[0]], ms[names[1]])]
    say(f"  history - default: {min(d) * 1e3:.1f}-{max(d) * 1e3:.1f} us per step (same-round pairs, "
        f"median {float(np.median(d)) * 1e3:.1f})")
    for name, (g, _, _) in steps.items():
        g.model.optimizer.check_status(dev)
        say(f"  {name}: loss after the timed steps {float(g.out['loss'].item()):.4f}")


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--out" in args:
        i = args.index("--out")
        OUT = args[i + 1]
        del args[i:i + 2]
    torch.cuda.set_device(dev)
    for part in args or ["kernels", "step"]:
        {"kernels": kernels, "step": step}[part]()
    with open(OUT, "w") as fh:
        fh.write("\n".join(_lines) + "\n")
