"""Model, batches and digests of tests/golden/bwd_layer_model_parent.json:
three GraphedTrainStep steps of a small model with the C3 step's tower widths
(query input 258 = 128 + 128 + 2, candidate input 212 = 128 + 64 + 16 + 4,
towers [256] -> 128, logQ in-batch softmax, Adagrad; B = 256), as the commit
named in the fixture computed them before each Dense layer's backward became
one launch.  Shared by tests/test_bwd_layer_model_gpu.py and
tests/golden/make_bwd_layer_model_golden.py that recorded the fixture.
"""
import functools
import hashlib
import json
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bwd_layer_model_parent.json")
B, STEPS, VOCAB = 256, 3, 300
QUERY = (("cust", 128), ("club", 128), ("news", 2))
CAND = (("art", 128), ("ptype", 64), ("colour", 16), ("dept", 4))


def _digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(dev):
    """{name: sha256} of the three losses and of every dense buffer, table and
    Adagrad accumulator after the three steps."""
    import torch

    from pkg import dtypes
    from pkg.modelling.models.two_tower_model import GraphedTrainStep, TwoTowerModel
    from pkg.modelling.optimizer_factory import OptimizerFactory
    from pkg.schema.features import Feature, FeatureFamily

    V = [str(i) for i in range(VOCAB)]
    qf = [Feature(n, dtypes.string, FeatureFamily.QUERY, embedding_size=d, vocab=V) for n, d in QUERY]
    cf = [Feature(n, dtypes.string, FeatureFamily.CANDIDATE, embedding_size=d, vocab=V) for n, d in CAND]
    rng = np.random.default_rng(41)
    probs = {str(i): float(p) for i, p in enumerate(rng.dirichlet(np.ones(VOCAB)))}
    m = TwoTowerModel(qf, cf, "art", 128, [256], [256], probs, device=dev, seed=3)
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", {"learning_rate": 0.05}))
    assert m.query_tower.dense.layout[0][1] == 258 and m.candidate_tower.dense.layout[0][1] == 212

    def batch():
        return {n: torch.as_tensor((rng.zipf(1.3, B) % (VOCAB + 1)).astype(np.int32), device=dev)
                for n, _ in QUERY + CAND}

    batches = [batch() for _ in range(STEPS + 1)]
    step = GraphedTrainStep(m, batches[0], warmup=1)
    out = {}
    for i, x in enumerate(batches[1:]):
        out[f"loss{i}"] = _digest(step(x)["loss"])
    torch.cuda.synchronize()
    for t, name in ((m.query_tower, "q"), (m.candidate_tower, "c")):
        out[name + ".mlp"] = _digest(t.dense.flat)
        out[name + ".mlp_acc"] = _digest(m.optimizer._slot(t.dense.flat, 1, 0.1)[0])
        for n, layer in t.input_layer.embedding_layers.items():
            out[f"{name}.{n}"] = _digest(layer.weight)
            out[f"{name}.{n}.acc"] = _digest(m.optimizer._slot(layer.weight, 1, 0.1)[0])
    m.optimizer.check_status(dev)
    return out


@functools.lru_cache(maxsize=None)
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)
