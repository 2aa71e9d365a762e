"""Cost of the Adam train step at the C3 shape (main.py schema, emb 128, towers
[256] -> 128, logQ in-batch softmax, B = 16384), Adam lr 1e-3:

  (a) eager, host step   train_step with the step count on the host: one
                         scale2_kernel and one adam_var_kernel per table, the
                         coefficients computed by the host (the only Adam path
                         before the device clock, unchanged by it: the baseline)
  (b) graphed Adam       GraphedTrainStep: Adam.enable_device_clock, one
                         adam_clock_advance, one dense launch, the whole-table
                         stages of all tables of a sparse call in one launch each
  (c) graphed Adagrad    the default step, for context

One process, three models on the same batches, warm; the variants alternate
in windows of STEPS steps (wall clock around a synchronised window, host time
included: that is what a training loop pays), ROUNDS rounds; ms/step as
min-max with the median, and (a) / (b) over same-round pairs.

  time_adam.py [--out PATH]                 the timing above -> profiles/adam_graphed_cost.txt
  time_adam.py --trace eager|graphed N      warm-up, then N steps of one variant, for a
                                            `rocprofv3 --kernel-trace --stats` run
  time_adam.py --summarize DIR_N1 N1 DIR_N2 N2 LABEL [ELEMENTS] [--out PATH]
                                            launches per step and time per launch of every kernel
                                            from two such runs of N1 < N2 steps (the difference
                                            drops warm-up and capture), appended to the output
                                            file, with the whole-table kernels' bytes/s from the
                                            tables' shapes (ELEMENTS: the tables' element count as
                                            the timing run printed it; default: from a model built
                                            here)."""
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

B = 16384
STEPS, ROUNDS = 20, 7
HBM_PEAK = 8.0e12  # bytes/s, MI355X specification
dev = torch.device("cuda:0")
OUT = os.path.join(ROOT, "profiles", "adam_graphed_cost.txt")
WHOLE_TABLE = {"scale2_kernel": "decay", "adam_var_kernel": "update", "adam_decay_many_kernel": "decay",
               "adam_var_many_kernel": "update"}
_lines = []


def say(line: str) -> None:
    print(line, flush=True)
    _lines.append(line)


def build(optimizer: str, lr: float):
    from pkg.modelling.models.two_tower_model import TwoTowerModel
    from pkg.modelling.optimizer_factory import OptimizerFactory

    schema = bench.main_schema()
    data = bench.SyntheticHM(dev, seed=1234)
    schema.set_candidate_prob_lookup(data.prob_lookup())
    model = TwoTowerModel.create_from_schema(schema, "article_id", device=dev, seed=0)
    model.compile(optimizer=OptimizerFactory.get_optimizer(optimizer, {"learning_rate": lr}))
    return model, data


def table_elements(model) -> int:
    return sum(layer.weight.numel() for t in model.towers for layer in t.input_layer.embedding_layers.values())


def variant(name: str, pool):
    """(callable running step i, model) of one variant, warmed."""
    from pkg.modelling.models.two_tower_model import GraphedTrainStep

    model, _ = build("adagrad" if name == "graphed adagrad" else "adam", 0.05 if name == "graphed adagrad" else 1e-3)
    if name == "eager adam":
        run = lambda i: model.train_step(pool[i % len(pool)])  # noqa: E731
    else:
        step = GraphedTrainStep(model, pool[0], warmup=2)
        packed = [step.pack(b) for b in pool]
        run = lambda i: step(packed=packed[i % len(packed)])  # noqa: E731
    for i in range(4):
        run(i)
    torch.cuda.synchronize()
    return run, model


def timing() -> None:
    data = bench.SyntheticHM(dev, seed=1234)
    pool = [data.batch(B) for _ in range(4)]
    names = ["eager adam", "graphed adam", "graphed adagrad"]
    runs = {}
    for n in names:
        runs[n], model = variant(n, pool)
        if n == "eager adam":
            elems = table_elements(model)
    say(f"C3 train step, B = {B}, Adam lr 1e-3 (Adagrad lr 0.05); {elems} table elements "
        f"({elems * 4 / 1e6:.0f} MB per table-shaped buffer); windows of {STEPS} steps, {ROUNDS} alternating rounds")
    ms = {n: [] for n in names}
    for _ in range(ROUNDS):
        for n in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(STEPS):
                runs[n](i)
            torch.cuda.synchronize()
            ms[n].append((time.perf_counter() - t0) * 1e3 / STEPS)
    for label, n in zip("abc", names):
        v = ms[n]
        say(f"  ({label}) {n}: {min(v):.3f}-{max(v):.3f} ms/step (median {float(np.median(v)):.3f})")
    gain = [x - y for x, y in zip(ms["eager adam"], ms["graphed adam"])]
    ratio = [x / y for x, y in zip(ms["eager adam"], ms["graphed adam"])]
    spread = max(max(ms[n]) - min(ms[n]) for n in names[:2])
    say(f"  (a) - (b), same-round pairs: {min(gain):.3f}-{max(gain):.3f} ms/step (median {float(np.median(gain)):.3f}); "
        f"(a) / (b): {min(ratio):.2f}-{max(ratio):.2f}x; largest spread of (a) or (b) over the rounds: {spread:.3f} ms")
    say(f"  (b) faster than (a) by more than that spread: {'yes' if min(gain) > spread else 'NO'}")


def trace(name: str, steps: int) -> None:
    data = bench.SyntheticHM(dev, seed=1234)
    pool = [data.batch(B) for _ in range(4)]
    run, _ = variant(f"{name} adam", pool)
    for i in range(steps):
        run(i)
    torch.cuda.synchronize()


def read_stats(directory: str) -> dict:
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    out = {}
    with open(files[-1]) as f:
        for r in csv.DictReader(f):
            out[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    return out


def short_name(name: str) -> str:
    """A kernel's name without namespaces, template and call arguments."""
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return name.split("(")[0].split("<")[0].split("::")[-1]


def summarize(dir1: str, n1: int, dir2: str, n2: int, label: str, elems: int) -> None:
    a, b = read_stats(dir1), read_stats(dir2)
    say(f"{label}: kernels per step from rocprofv3 --kernel-trace --stats runs of {n1} and {n2} steps "
        "(their difference, per step)")
    total, rows = 0.0, []
    for name, (calls, ns) in b.items():
        c0, ns0 = a.get(name, (0, 0.0))
        per_step = (calls - c0) / (n2 - n1)
        if per_step <= 0:
            continue
        total += per_step
        rows.append((per_step, (ns - ns0) / max(calls - c0, 1), name))
    say(f"  launches per step: {total:.1f}")
    for per_step, avg_ns, name in sorted(rows, key=lambda r: -r[0] * r[1])[:12]:
        line = f"  {per_step:5.1f} x {avg_ns / 1e3:9.1f} us  {short_name(name)}"
        kind = next((k for k in WHOLE_TABLE if k in name), None)
        if kind:
            # per step the stage moves all tables' elements x 4 B x 4 accesses
            # (decay: m, v read and written; update: var read and written, m, v read)
            bps = elems * 4 * 4 / (per_step * avg_ns * 1e-9)
            line += f"   [{WHOLE_TABLE[kind]}: {elems * 16 / 1e9:.2f} GB per step, {bps / 1e12:.2f} TB/s, " \
                    f"{100 * bps / HBM_PEAK:.0f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak]"
        say(line)


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--out" in args:
        i = args.index("--out")
        OUT = args[i + 1]
        del args[i:i + 2]
    if args[:1] != ["--summarize"] or len(args) <= 6:  # a summary with ELEMENTS given needs no GPU
        torch.cuda.set_device(dev)
    if args[:1] == ["--trace"]:
        trace(args[1], int(args[2]))
    elif args[:1] == ["--summarize"]:
        elements = int(args[6]) if len(args) > 6 else table_elements(build("adam", 1e-3)[0])
        summarize(args[1], int(args[2]), args[3], int(args[4]), args[5], elements)
        with open(OUT, "a") as fh:
            fh.write("\n".join(_lines) + "\n")
    else:
        timing()
        with open(OUT, "w") as fh:
            fh.write("\n".join(_lines) + "\n")
