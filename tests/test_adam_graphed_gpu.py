"""GPU: Adam in the graphed and device-resident train step.

GraphedTrainStep, fit(use_graph=True), the device-resident fit and
modelling_runner with the Adam optimizer: the captured step (step count and
coefficients on the device, Adam.enable_device_clock) against the eager step
with the host step count, bit for bit — losses, tables, both slots of every
table and of both MLP buffers, and the iteration count.

Tiny models: B = 256, a handful of small tables, towers [68] -> 32.
"""
import os

import numpy as np
import pytest
import torch

from pkg import dtypes
from pkg.modelling import hip_ops
from pkg.modelling.dataset import CandidateCatalogue, DeviceDataset, EncodedDataset
from pkg.modelling.models.two_tower_model import GraphedTrainStep, TwoTowerModel
from pkg.modelling.optimizer_factory import Adagrad, Adam, OptimizerFactory
from pkg.schema.features import Feature, FeatureFamily

pytestmark = pytest.mark.gpu

B, E, H, L, HV = 256, 32, 68, 5, 50
V = [str(i) for i in range(600)]
ADAM_OPS = ["adam_coef_len", "adam_coef_tables", "adam_clock_advance", "dense_adam_many_dev", "sparse_adam_dev",
            "dense_adam", "sparse_adam"]


def _features(history=False):
    qf = [Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=16, vocab=V[:300]),
          Feature("post", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V[:50])]
    if history:
        qf.append(Feature("hist", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V[:HV],
                          sequence_length=L, pooling="mean"))
    cf = [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=16, vocab=V),
          Feature("price", dtypes.float32, FeatureFamily.CANDIDATE),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=V[:20])]
    return qf, cf


def _model(cuda, seed, optimizer, history=False, **kw):
    qf, cf = _features(history)
    probs = {v: float(p) for v, p in zip(V, np.random.default_rng(seed).dirichlet(np.ones(len(V))))}
    m = TwoTowerModel(qf, cf, "art", E, [H], [H], probs, device=cuda, seed=seed, **kw)
    m.compile(optimizer=optimizer)
    return m


def _columns(rng, n, history=False):
    cols = {"cust": rng.integers(0, 301, n).astype(np.int32), "post": rng.integers(0, 51, n).astype(np.int32),
            "art": (rng.zipf(1.3, n) % 301).astype(np.int32), "ptn": rng.integers(0, 21, n).astype(np.int32),
            "price": rng.uniform(0, 1, n).astype(np.float32)}
    if history:
        ids = rng.integers(0, HV + 1, (n, L)).astype(np.int32)
        ids[np.arange(L)[None, :] >= rng.integers(0, L + 1, n)[:, None]] = -1
        cols["hist"] = ids
    return cols


def _batch(cuda, rng, n=B, history=False):
    return {k: torch.as_tensor(v, device=cuda) for k, v in _columns(rng, n, history).items()}


def _state(m):
    """MLP buffers, tables and every optimizer slot of both."""
    adam = isinstance(m.optimizer, Adam)
    slots = (lambda p: m.optimizer._slot(p, 2, 0.0)) if adam else (lambda p: m.optimizer._slot(p, 1, 0.1))
    out = {}
    for t, name in ((m.query_tower, "q"), (m.candidate_tower, "c")):
        out[name + ".mlp"] = t.dense.flat.detach().clone()
        for i, s in enumerate(slots(t.dense.flat)):
            out[f"{name}.mlp.slot{i}"] = s.clone()
        for n, layer in t.input_layer.embedding_layers.items():
            out[f"{name}.{n}"] = layer.weight.detach().clone()
            for i, s in enumerate(slots(layer.weight)):
                out[f"{name}.{n}.slot{i}"] = s.clone()
    return out


def _assert_same_state(a, b, where=""):
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (where, k)


def _graphed_against_eager(cuda, a, b, batches):
    """`a` steps eagerly, `b` through one GraphedTrainStep (warm-up = batch 0)."""
    want = [a.train_step(x)["loss"].clone() for x in batches]
    assert all(bool(torch.isfinite(w)) for w in want), want
    g = GraphedTrainStep(b, batches[0], warmup=1)
    got = [g.warmup_out["loss"].clone()] + [g(x)["loss"].clone() for x in batches[1:]]
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(got, want)):
        assert torch.isfinite(x) and torch.equal(x, y), i
    _assert_same_state(a, b)
    return g


def test_graphed_step_equals_eager_host_step(cuda):
    rng = np.random.default_rng(1)
    batches = [_batch(cuda, rng) for _ in range(5)]
    a, b = _model(cuda, 2, Adam(1e-3)), _model(cuda, 2, Adam(1e-3))
    before = _state(a)
    g = _graphed_against_eager(cuda, a, b, batches)
    assert a.optimizer._clock is None and b.optimizer._clock is not None
    assert a.optimizer.iterations == 5 and b.optimizer.iterations == 5
    after = _state(a)
    assert all(not torch.equal(before[k], after[k]) for k in before)  # every buffer and slot moved
    assert g.reusable(b, batch=batches[0])
    # the device word is the count: an eager step of the graphed model continues from it
    la, lb = a.train_step(batches[0])["loss"], b.train_step(batches[0])["loss"]
    assert torch.equal(la, lb) and b.optimizer.iterations == 6
    _assert_same_state(a, b, "eager step after the replays")
    b.optimizer.iterations = 2
    assert b.optimizer.iterations == 2


def test_graphed_fit_on_a_device_dataset(cuda):
    """3 full batches and a partial one, 2 epochs: replays, the eager
    remainder and the second epoch all continue one step count."""
    cols = _columns(np.random.default_rng(3), 3 * B + 100)
    a, b = _model(cuda, 4, Adam(1e-3)), _model(cuda, 4, Adam(1e-3))
    ha = a.fit(EncodedDataset(cols, B, 300, seed=9, device=cuda), epochs=2, use_graph=False)
    hb = b.fit(DeviceDataset(cols, B, 300, seed=9, device=cuda), epochs=2, use_graph=True)
    torch.cuda.synchronize()
    assert b._device_fit_graph is not None and b.optimizer._clock is not None
    np.testing.assert_allclose(hb["loss"], ha["loss"], rtol=1e-12)
    assert a.optimizer.iterations == 8 and b.optimizer.iterations == 8
    _assert_same_state(a, b)


def test_graphed_fit_on_host_batches(cuda):
    """fit(use_graph=True) over an EncodedDataset: warm-up, replays, eager partial batch."""
    cols = _columns(np.random.default_rng(5), 2 * B + 50)
    a, b = _model(cuda, 6, Adam(1e-3)), _model(cuda, 6, Adam(1e-3))
    ha = a.fit(EncodedDataset(cols, B, device=cuda), epochs=2, use_graph=False)
    hb = b.fit(EncodedDataset(cols, B, device=cuda), epochs=2, use_graph=True)
    torch.cuda.synchronize()
    np.testing.assert_allclose(hb["loss"], ha["loss"], rtol=1e-12)
    assert a.optimizer.iterations == 6 and b.optimizer.iterations == 6
    _assert_same_state(a, b)


def test_every_option_together(cuda):
    """A sequence feature, mixed negatives (the towers' batches differ: B and
    B + M rows), accidental hits, cosine scoring with a temperature and sample
    weights."""
    M = 40
    rng = np.random.default_rng(7)
    crng = np.random.default_rng(42)
    cat_cols = {"art": np.arange(101, 601).astype(np.int32), "price": crng.uniform(0, 1, 500).astype(np.float32),
                "ptn": crng.integers(0, 21, 500).astype(np.int32)}

    def build():
        m = _model(cuda, 8, Adam(1e-3), history=True, num_sampled_negatives=M, sampled_negatives_seed=11,
                   remove_accidental_hits=True, normalize_embeddings=True, temperature=0.1)
        m.set_candidate_catalogue(CandidateCatalogue(cat_cols, _features(True)[1], device=cuda))
        m.sample_weight_scale = 2.0
        return m

    batches = []
    for _ in range(3):
        x = _batch(cuda, rng, history=True)
        x["__weight__"] = torch.as_tensor(rng.uniform(0.05, 1.0, B).astype(np.float32), device=cuda)  # w / w_max
        batches.append(x)
    a, b = build(), build()
    _graphed_against_eager(cuda, a, b, batches)
    assert a.optimizer.iterations == 3 and b.optimizer.iterations == 3
    assert int(b._mixed_step.item()) == 3
    assert len(b.query_tower.input_layer.bag_sources()) == 1


def test_saturation_crossing(cuda):
    """betas (0.5, 0.75): the coefficient table ends at step 61; steps 59..64
    cross its end (the clock clamps, the host keeps calling powf)."""
    def opt():
        o = Adam(1e-3, beta_1=0.5, beta_2=0.75)
        o.iterations = 58
        return o

    assert hip_ops.adam_coef_len(0.5, 0.75) == 61
    rng = np.random.default_rng(9)
    batches = [_batch(cuda, rng) for _ in range(6)]
    a, b = _model(cuda, 10, opt()), _model(cuda, 10, opt())
    _graphed_against_eager(cuda, a, b, batches)
    assert a.optimizer.iterations == 64 and b.optimizer.iterations == 64
    assert b.optimizer._coef_tables[0].numel() == 61


def test_beta_without_a_table_is_refused_for_capture_only(cuda):
    m = _model(cuda, 11, Adam(1e-3, beta_2=1.0))
    x = _batch(cuda, np.random.default_rng(12))
    with pytest.raises(ValueError, match="beta_2=1.0"):
        GraphedTrainStep(m, x, warmup=1)
    assert m.optimizer._clock is None
    assert torch.isfinite(m.train_step(x)["loss"]) and m.optimizer.iterations == 1  # eager still runs

    class Other:
        learning_rate = 0.1

    m.compile(optimizer=Other())
    with pytest.raises(ValueError, match="Adagrad or the Adam"):
        GraphedTrainStep(m, x, warmup=1)


def _count(monkeypatch, names):
    calls = {n: 0 for n in names}

    def counted(name):
        fn = getattr(hip_ops, name)

        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper

    for n in names:
        monkeypatch.setattr(hip_ops, n, counted(n))
    return calls


def test_adagrad_graphed_step_is_unchanged_and_calls_no_adam_entry(cuda, monkeypatch):
    calls = _count(monkeypatch, ADAM_OPS)
    rng = np.random.default_rng(13)
    batches = [_batch(cuda, rng) for _ in range(3)]
    a, b = _model(cuda, 14, Adagrad(0.05)), _model(cuda, 14, Adagrad(0.05))
    _graphed_against_eager(cuda, a, b, batches)
    assert a.optimizer.iterations == 3  # Adagrad's count stays on the host: replays do not reach it
    assert calls == {n: 0 for n in ADAM_OPS}


def test_launches_per_step(cuda, monkeypatch):
    """Without enable_device_clock Adam calls what it always called; with it a
    step is one advance, one dense launch and one sparse call for both towers
    (one per tower when their batches differ)."""
    calls = _count(monkeypatch, ADAM_OPS)
    x = _batch(cuda, np.random.default_rng(15))
    m = _model(cuda, 16, Adam(1e-3))
    m.train_step(x)
    assert calls == dict.fromkeys(ADAM_OPS, 0) | {"dense_adam": 2, "sparse_adam": 2}
    m.optimizer.enable_device_clock(cuda)
    m.optimizer.enable_device_clock(cuda)  # a no-op
    assert (calls["adam_coef_len"], calls["adam_coef_tables"]) == (1, 1)
    assert m.optimizer.iterations == 1
    m.train_step(x)
    assert m.optimizer.iterations == 2
    assert calls == {"adam_coef_len": 1, "adam_coef_tables": 1, "adam_clock_advance": 1, "dense_adam_many_dev": 1,
                     "sparse_adam_dev": 1, "dense_adam": 2, "sparse_adam": 2}


def test_modelling_runner_with_adam(cuda, tmp_path):
    import pandas as pd

    from pkg.modelling.dataset import encode_dataframe
    from pkg.modelling.runner import modelling_runner
    from pkg.schema.model_config import ModelConfig
    from pkg.schema.schema import Schema
    from pkg.schema.training_config import TrainingConfig
    from pkg.utils.settings import Settings

    rng = np.random.default_rng(0)
    n = 1500
    df = pd.DataFrame({"customer_id": rng.integers(0, 200, n).astype(str),
                       "article_id": (rng.zipf(1.3, n) % 400).astype(str),
                       "section": rng.integers(0, 7, n).astype(str)})
    feats = [Feature("customer_id", dtypes.string, FeatureFamily.QUERY, embedding_size=16),
             Feature("article_id", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=16),
             Feature("section", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=4)]
    schema = Schema(feats, TrainingConfig(256, 512, "adam", {"learning_rate": 1e-3}, candidate_batch_size=128,
                                          epochs=2), ModelConfig(16, [1, 10], [32], [32]))
    train, test = df.iloc[:1200], df.iloc[1200:]
    schema.build_features_from_dataframe(train)
    probs = train["article_id"].value_counts() / len(train)
    schema.set_candidate_prob_lookup({str(k): float(v) for k, v in probs.items()})
    cands = df.drop_duplicates("article_id")
    d = str(tmp_path)
    s = Settings("", "", "", ("", ""), ("", ""), ("", ""), "t_dat", "article_id", f"{d}/cand/c", "", "",
                 f"{d}/train/t", f"{d}/test/t", f"{d}/schema.pkl", f"{d}/model/", f"{d}/index/i", f"{d}/base/b")
    schema.save(s.schema_filepath)
    for part, path in ((train, "train"), (test, "test")):
        EncodedDataset(encode_dataframe(part, feats), device=cuda).save(f"{d}/{path}")
    EncodedDataset(encode_dataframe(cands, schema.candidate_features), device=cuda).save(f"{d}/cand")
    model = modelling_runner(s)  # use_graph=True, device_resident=True
    assert isinstance(model.optimizer, Adam) and model.optimizer._clock is not None
    assert model._device_fit_graph is not None
    assert model.optimizer.iterations == 2 * 5  # 4 full batches of 256 and one of 176, two epochs
    assert os.path.exists(f"{d}/model/two_tower.pt")
    assert all(bool(torch.isfinite(v).all()) for v in model.state_dict().values())
