"""The kernel launches of one eager and one graphed train step of the tests'
small two-tower model (vocab 300, hidden 64, joint 32, logQ, Adagrad, B = 256),
to compare two trees launch for launch, and the eager step's host time.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/step_launches.py run
      (a kernel trace on its own: no counter collection beside it)
  python tools/step_launches.py compare PARENT_kernel_trace.csv CHANGE_kernel_trace.csv
      prints both trees' lists (kernel name, grid, workgroup size; per queue in
      dispatch order) of the eager step and of the graph replay, and whether
      they are equal per queue and as name-sorted multisets
  python tools/step_launches.py time [--steps 300 --warmup 20]
      ms per eager train_step (host-bound at this size), one figure per line

`run` brackets each step with a 4M-element torch fill, which no launch of the
small model resembles; `compare` cuts the trace at those.
"""
import argparse
import csv
import os
import sys
import time
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

MARK = 4_000_000
SECTIONS = ("eager step", "graph replay")


def small_model(dev, fused=False):
    import numpy as np
    from pkg import dtypes
    from pkg.modelling.models.two_tower_model import TwoTowerModel
    from pkg.modelling.optimizer_factory import OptimizerFactory
    from pkg.schema.features import Feature, FeatureFamily

    V = [str(i) for i in range(300)]
    qf = [Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=16, vocab=V),
          Feature("post", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V[:50])]
    cf = [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=16, vocab=V),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=V[:20]),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=4, vocab=V[:20])]
    probs = {str(i): float(p) for i, p in enumerate(np.random.default_rng(0).dirichlet(np.ones(300)))}
    m = TwoTowerModel(qf, cf, "art", 32, [64], [64], probs, device=dev, seed=0, fused_optimizer_apply=fused)
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", {"learning_rate": 0.05}))
    return m


def batch(dev, B=256):
    import numpy as np
    import torch

    rng = np.random.default_rng(1)
    z = lambda v: torch.as_tensor((rng.zipf(1.3, B) % v).astype(np.int32), device=dev)  # noqa: E731
    return {"cust": z(301), "post": z(51), "art": z(301), "ptn": z(21)}


def run(a):
    import torch
    from pkg.modelling.models.two_tower_model import GraphedTrainStep

    dev = torch.device("cuda:0")
    m, x = small_model(dev, a.fused), batch(dev)
    for _ in range(3):
        m.train_step(x)
    g = GraphedTrainStep(m, x, warmup=1)
    torch.cuda.synchronize()

    def mark():
        torch.cuda.synchronize()
        torch.full((MARK,), 1.0, device=dev)
        torch.cuda.synchronize()

    mark()
    m.train_step(x)
    mark()
    g.replay()
    mark()
    print("loss", float(g.out["loss"]))


def sections(path):
    """{section: {queue: [(name, grid, workgroup)] in dispatch order}}."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    dims = lambda r, k: "x".join(r[f"{k}_{d}"] for d in "XYZ")  # noqa: E731
    marks = [i for i, r in enumerate(rows) if "FillFunctor" in r["Kernel_Name"] and int(r["Grid_Size_X"]) >= MARK // 64]
    if len(marks) != len(SECTIONS) + 1:
        raise SystemExit(f"{path}: {len(marks)} marker launches, expected {len(SECTIONS) + 1}")
    out = {}
    for name, lo, hi in zip(SECTIONS, marks, marks[1:]):
        queues = {}
        for r in rows[lo + 1:hi]:
            queues.setdefault(r["Queue_Id"], []).append((r["Kernel_Name"], dims(r, "Grid_Size"), dims(r, "Workgroup_Size")))
        out[name] = queues
    return out


def compare(a):
    trees = {"parent": sections(a.parent), "change": sections(a.change)}
    verdicts = []
    for sec in SECTIONS:
        per_queue, flat = {}, {}
        for tree, secs in trees.items():
            # queue ids are the runtime's: queues are told apart by what they ran
            per_queue[tree] = sorted(tuple(q) for q in secs[sec].values())
            flat[tree] = sorted(k for q in secs[sec].values() for k in q)
            print(f"== {sec}, {tree}: {len(flat[tree])} launches on {len(per_queue[tree])} queues")
            for qi, q in enumerate(per_queue[tree]):
                for name, grid, wg in q:
                    print(f"  q{qi}  grid {grid:<14} wg {wg:<10} {name}")
        same_q = per_queue["parent"] == per_queue["change"]
        same_m = Counter(flat["parent"]) == Counter(flat["change"])
        verdicts.append(f"{sec}: per-queue ordered lists {'EQUAL' if same_q else 'DIFFER'}; name-sorted multiset "
                        f"{'EQUAL' if same_m else 'DIFFERS'} ({len(flat['parent'])} vs {len(flat['change'])} launches)")
    print("== verdict")
    print("\n".join(verdicts))


def timing(a):
    import torch

    dev = torch.device("cuda:0")
    m, x = small_model(dev, a.fused), batch(dev)
    for _ in range(a.warmup):
        m.train_step(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        m.train_step(x)
    torch.cuda.synchronize()
    print(f"eager_ms_per_step {(time.perf_counter() - t0) / a.steps * 1e3:.4f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("run", "time"):
        p = sub.add_parser(name)
        p.add_argument("--fused", action="store_true", help="fused_optimizer_apply")
        p.add_argument("--steps", type=int, default=300)
        p.add_argument("--warmup", type=int, default=20)
    p = sub.add_parser("compare")
    p.add_argument("parent")
    p.add_argument("change")
    a = ap.parse_args()
    {"run": run, "compare": compare, "time": timing}[a.cmd](a)
