"""Cost of the accidental-hit mask: the fused in-batch entry at the benched
operating point (16384 x 16384 x 128, article ids Zipf(1.1) over 105,542 as
bench.py draws them) with and without ids, bf16 and x3.  Device events around
REPS back-to-back calls, warm, the four variants interleaved over ROUNDS
rounds; prints each variant's range and the hits / plain ratios, and the
share of masked pairs of the batch (a host count)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from pkg.modelling import hip_ops  # noqa: E402

B, E, V = 16384, 128, bench.HM_VOCAB["article_id"]
REPS, ROUNDS = 20, 5
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
p = bench.zipf_probs(V, 1.1)
art = rng.choice(V, size=B, p=p).astype(np.int32)
counts = np.bincount(art, minlength=V).astype(np.int64)
masked = int((counts * (counts - 1)).sum())  # ordered pairs (i, j != i) of equal id
print(f"batch {B}: {int((counts > 0).sum())} distinct articles, {masked} masked pairs = "
      f"{masked / (B * (B - 1)):.4%} of the off-diagonal pairs, "
      f"{int((counts[art] > 1).sum()) / B:.1%} of the rows have at least one", flush=True)

g = torch.Generator(device=dev)
g.manual_seed(0)
table = torch.randn(V, E, generator=g, device=dev) * 0.3
ids = torch.as_tensor(art, device=dev)
c = table[ids.long()].contiguous()
q = torch.randn(B, E, generator=g, device=dev) * 0.3
logq = torch.as_tensor(np.log(p).astype(np.float32), device=dev)[ids.long()].contiguous()

variants = {"bf16 plain": dict(x3=False), "bf16 hits": dict(x3=False, ids=ids), "x3 plain": dict(x3=True),
            "x3 hits": dict(x3=True, ids=ids)}
for kw in variants.values():  # warm: workspaces, kernel attributes
    for _ in range(3):
        hip_ops.inbatch_fused(q, c, logq, **kw)
torch.cuda.synchronize()
ms = {k: [] for k in variants}
for _ in range(ROUNDS):
    for name, kw in variants.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            hip_ops.inbatch_fused(q, c, logq, **kw)
        b.record()
        b.synchronize()
        ms[name].append(a.elapsed_time(b) / REPS)
for name, v in ms.items():
    print(f"{name}: {min(v) * 1e3:.1f}-{max(v) * 1e3:.1f} us per call (median {float(np.median(v)) * 1e3:.1f})")
for kind in ("bf16", "x3"):
    r = [h / pl for h, pl in zip(ms[f"{kind} hits"], ms[f"{kind} plain"])]
    print(f"{kind} hits / plain: {min(r):.3f}-{max(r):.3f} (same-round pairs)")
print(f"x3 plain / bf16 plain: {np.median(ms['x3 plain']) / np.median(ms['bf16 plain']):.2f}")
