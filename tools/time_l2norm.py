"""Cost and precision of cosine scoring (normalize_embeddings / temperature).

  kernels  tt_l2norm_rows and tt_l2norm_rows_grad, one launch each over both
           towers' operands (2 x 16384 x 128 fp32), against a device copy that
           moves the same bytes (the copy_floor idea of the gather roofline):
           the forward reads and writes 16 MiB (a copy of 16 MiB), the
           gradient reads 32 MiB and writes 16 MiB (a copy of 24 MiB).
  step     the graphed C3 train step (bench.py's model and batches) with and
           without normalize_embeddings=True, temperature=0.05.
  drift    the DEFAULT bf16 in-batch entry's dQ / dC / loss against torch fp64
           (relative 2-norm, as DESIGN §6's table) on the C3 model's own tower
           outputs after 4 Adagrad steps: un-normalised (the §6 baseline) and
           normalised at T = 1 and T = 0.05; the x3 entry beside it.

Device events around REPS back-to-back calls (the kernels: replayed from one
hipGraph per variant, so no host time sits between the launches), warm, the
variants interleaved over ROUNDS rounds; ranges printed.  Usage: time_l2norm.py [kernels step drift]."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from pkg.modelling import hip_ops  # noqa: E402
from pkg.modelling.models.two_tower_model import GraphedTrainStep, TwoTowerModel  # noqa: E402
from pkg.modelling.optimizer_factory import OptimizerFactory  # noqa: E402

B, E = 16384, 128
REPS, ROUNDS = 50, 7
dev = torch.device("cuda:0")


def interleaved(variants: dict, reps: int = REPS, rounds: int = ROUNDS) -> dict:
    """ms per call of each variant: warm, then `rounds` rounds of every
    variant in turn, `reps` back-to-back calls between two device events."""
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
    """`reps` calls of fn as one hipGraph: a replay has no host work between
    the launches (the wrappers' Python costs more than these kernels run)."""
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
        print(f"  {name}: {min(v) * 1e3:.1f}-{max(v) * 1e3:.1f} us per call (median {float(np.median(v)) * 1e3:.1f})",
              flush=True)


def kernels() -> None:
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    x = [torch.relu(torch.randn(B, E, generator=g, device=dev)) for _ in range(2)]
    dy = [torch.randn(B, E, generator=g, device=dev) for _ in range(2)]
    y = [torch.empty_like(t) for t in x]
    dx = [torch.empty_like(t) for t in x]
    inv = [torch.empty(B, device=dev) for _ in range(2)]
    scale = (20.0, 1.0)
    nbytes = 2 * B * E * 4
    src16, dst16 = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    src24, dst24 = (torch.empty(nbytes * 3 // 2, dtype=torch.uint8, device=dev) for _ in range(2))
    calls = {
        "l2norm_rows (2 jobs)": lambda: hip_ops.l2norm_rows([(x[i], scale[i], y[i], inv[i]) for i in range(2)]),
        "copy 16 MiB": lambda: dst16.copy_(src16),
        "l2norm_rows_grad (2 jobs)": lambda: hip_ops.l2norm_rows_grad(
            [(x[i], inv[i], dy[i], scale[i], dx[i]) for i in range(2)]),
        "l2norm_rows_grad in place": lambda: hip_ops.l2norm_rows_grad(
            [(x[i], inv[i], dx[i], scale[i], dx[i]) for i in range(2)]),
        "copy 24 MiB": lambda: dst24.copy_(src24),
    }
    graphs = {k: graphed(fn, REPS) for k, fn in calls.items()}  # keep the graphs alive while they replay
    ms = {k: [t / REPS for t in v] for k, v in interleaved({k: g.replay for k, g in graphs.items()}, reps=1).items()}
    print(f"kernels at 2 x {B} x {E} fp32 ({nbytes >> 20} MiB per pass over both operands):")
    show(ms)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for k, c, moved in (("l2norm_rows (2 jobs)", "copy 16 MiB", 2 * nbytes),
                        ("l2norm_rows_grad (2 jobs)", "copy 24 MiB", 3 * nbytes),
                        ("l2norm_rows_grad in place", "copy 24 MiB", 3 * nbytes)):
        r = [a / b for a, b in zip(ms[k], ms[c])]
        print(f"  {k} / {c}: {min(r):.2f}-{max(r):.2f} (same-round pairs); "
              f"{moved / med[k] / 1e9:.2f} TB/s of operand traffic at the median")


def c3_model(data, **kw):
    schema = bench.main_schema()
    schema.set_candidate_prob_lookup(data.prob_lookup())
    m = TwoTowerModel.create_from_schema(schema, "article_id", device=dev, seed=0, **kw)
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", {"learning_rate": 0.05}))
    return m


def step() -> None:
    data = bench.SyntheticHM(dev, seed=1234)
    pool = [data.batch(B) for _ in range(4)]
    steps = {}
    for name, kw in (("default", {}), ("cosine T=0.05", dict(normalize_embeddings=True, temperature=0.05))):
        g = GraphedTrainStep(c3_model(data, **kw), pool[0], warmup=2)
        packed = [g.pack(b) for b in pool]
        steps[name] = (g, packed, [0])

    def run(name):
        g, packed, i = steps[name]
        g(packed=packed[i[0] % len(packed)])
        i[0] += 1

    ms = interleaved({k: (lambda k=k: run(k)) for k in steps}, reps=100)
    print(f"graphed C3 train step, B = {B}:")
    show(ms)
    d = [b - a for a, b in zip(ms["default"], ms["cosine T=0.05"])]
    print(f"  cosine - default: {min(d) * 1e3:.1f}-{max(d) * 1e3:.1f} us per step (same-round pairs, "
          f"median {float(np.median(d)) * 1e3:.1f})")
    for name, (g, _, _) in steps.items():
        g.model.optimizer.check_status(dev)
        print(f"  {name}: loss after the timed steps {float(g.out['loss'].item()):.4f}")


def fp64_inbatch(q, c, logq, block=2048):
    """torch fp64 in-batch loss and gradients: row_loss [B], dq, dc."""
    qd, cd, ld = q.double(), c.double(), logq.double()
    n = qd.shape[0]
    dq, dc = torch.empty_like(qd), torch.zeros_like(cd)
    rl = torch.empty(n, dtype=torch.float64, device=q.device)
    for s in range(0, n, block):
        S = qd[s:s + block] @ cd.T - ld[None, :]
        lse = torch.logsumexp(S, 1)
        r = torch.arange(s, min(s + block, n), device=q.device)
        rl[s:s + block] = lse - S[r - s, r]
        P = torch.exp(S - lse[:, None])
        P[r - s, r] -= 1.0
        dq[s:s + block] = P @ cd
        dc += P.T @ qd[s:s + block]
    return rl, dq, dc


def drift() -> None:
    print("default bf16 in-batch entry against fp64 after 4 Adagrad steps at C3 (relative 2-norm; x3 beside it):")
    for name, kw in (("dot product (baseline)", {}), ("cosine T=1", dict(normalize_embeddings=True)),
                     ("cosine T=0.05", dict(normalize_embeddings=True, temperature=0.05))):
        data = bench.SyntheticHM(dev, seed=11)
        m = c3_model(data, **kw)
        for _ in range(4):
            m.train_step(data.batch(B))
        b = data.batch(B)
        with torch.no_grad():
            # the towers' outputs as the loss takes them (normalised and scaled under cosine scoring)
            q, c = (t.dense(t.input_layer({f.name: b[f.name] for f in t.input_layer.categorical_features}))
                    for t in m.towers)
            logq = m.candidate_logq(b)
            rl, dq_ref, dc_ref = fp64_inbatch(q, c, logq)
            smax = float((q.double() @ c.double()[:256].T).abs().max())
            dead = [int((t == 0).all(1).sum()) for t in (q, c)]
            out = {}
            for tag, x3 in (("bf16", False), ("x3", True)):
                _, row_loss, dq, dc = hip_ops.inbatch_fused(q.contiguous(), c.contiguous(), logq, x3=x3)
                out[tag] = (float((dq.double() - dq_ref).norm() / dq_ref.norm()),
                            float((dc.double() - dc_ref).norm() / dc_ref.norm()),
                            abs(float(row_loss.double().sum()) - float(rl.sum())) / float(rl.sum()))
        print(f"  {name}: max |S| {smax:.3g}, dead rows q {dead[0]} c {dead[1]}, loss {float(rl.sum()) / B:.4f}/row; "
              + "; ".join(f"{tag} dQ {v[0]:.2e} dC {v[1]:.2e} loss {v[2]:.1e}" for tag, v in out.items()),
              flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    torch.cuda.set_device(dev)
    for part in sys.argv[1:] or ["kernels", "step", "drift"]:
        {"kernels": kernels, "step": step, "drift": drift}[part]()
