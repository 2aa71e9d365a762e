"""GPU: a sequence feature ("the last L articles of this customer") through
the public interface: eager / fused / graphed training, fit from a
DeviceDataset, Adam, export and serving, and the absence of any new launch in
a model without one.

Tiny model: B = 96; query tower = one ordinary feature (dim 16) + one history
feature (L = 5, dim 8, vocab 50, mean pooling, some empty bags); ordinary
candidate tower; one hidden layer of 48, E = 32, logQ on.

The file's name sorts after the other GPU test files on purpose: these tests
create streams and capture graphs, and torch hands streams out round-robin
from a pool of 32, so running them earlier would change which streams the
later files' tests receive (test_model_gpu's capture_guard test expects its
two fresh streams to differ from the capture stream)."""
import numpy as np
import pytest
import torch

import bag_ref
from oracle import oracle
from pkg import dtypes
from pkg.modelling import hip_ops
from pkg.modelling.dataset import DeviceDataset, EncodedDataset
from pkg.modelling.export import Retriever
from pkg.modelling.indices.brute_force import BruteForceIndex
from pkg.modelling.models.two_tower_model import GraphedTrainStep, TwoTowerModel
from pkg.modelling.optimizer_factory import OptimizerFactory
from pkg.schema.features import Feature, FeatureFamily

pytestmark = pytest.mark.gpu

B, E, H, L, HV = 96, 32, 48, 5, 50


def _features(history=True, pooling="mean"):
    V = [str(i) for i in range(300)]
    qf = [Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=16, vocab=V)]
    if history:
        qf.append(Feature("hist", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V[:HV],
                          sequence_length=L, pooling=pooling))
    cf = [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=16, vocab=V),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=V[:20])]
    return qf, cf


def _model(cuda, seed=0, optimizer="adagrad", history=True, **kw):
    qf, cf = _features(history)
    probs = {str(i): float(p) for i, p in enumerate(np.random.default_rng(seed).dirichlet(np.ones(300)))}
    m = TwoTowerModel(qf, cf, "art", E, [H], [H], probs, device=cuda, seed=seed, **kw)
    lr = 0.05 if optimizer == "adagrad" else 1e-3
    m.compile(optimizer=OptimizerFactory.get_optimizer(optimizer, {"learning_rate": lr}))
    return m


def _hist(rng, n):
    """[n, L] int32 history ids: left-aligned, -1 padded, every length 0..L."""
    ids = rng.integers(0, HV + 1, (n, L)).astype(np.int32)
    length = rng.integers(0, L + 1, n)
    length[:3] = (0, L, 1)
    ids[np.arange(L)[None, :] >= length[:, None]] = -1
    return ids


def _columns(rng, n, history=True):
    cols = {"cust": rng.integers(0, 301, n).astype(np.int32), "art": rng.integers(0, 301, n).astype(np.int32),
            "ptn": rng.integers(0, 21, n).astype(np.int32)}
    if history:
        cols["hist"] = _hist(rng, n)
    return cols


def _batch(cuda, rng, n, history=True):
    return {k: torch.as_tensor(v, device=cuda) for k, v in _columns(rng, n, history).items()}


def _state(m):
    out = {}
    for t, name in ((m.query_tower, "q"), (m.candidate_tower, "c")):
        out[name + ".mlp"] = t.dense.flat.detach().clone()
        for n, layer in t.input_layer.embedding_layers.items():
            out[f"{name}.{n}"] = layer.weight.detach().clone()
            out[f"{name}.{n}.acc"] = m.optimizer._slot(layer.weight, 1, 0.1)[0].clone()
    return out


def _assert_same_state(a, b, where=""):
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (where, k)


def _fp64_loss(m, x):
    """torch fp64 restatement of the whole model: lookups, masked mean pooling,
    concat in declaration order, MLPs (ReLU after every layer), scores - logQ,
    CE-SUM with eye labels."""
    def tower_in(tower, feats):
        parts = []
        for f in feats:
            w = tower.input_layer.embedding_layers[f.name].weight.double()
            ids = x[f.name].long()
            if f.is_sequence:
                ok = (ids >= 0) & (ids < w.shape[0])
                rows = w[torch.where(ok, ids, torch.zeros_like(ids))] * ok[..., None]
                cnt = ok.sum(1, keepdim=True).double()
                parts.append(torch.where(cnt > 0, rows.sum(1) / cnt.clamp_min(1.0), torch.zeros_like(rows.sum(1))))
            else:
                parts.append(w[ids])
        return torch.cat(parts, 1)

    outs = []
    for tower, feats in ((m.query_tower, m.query_features), (m.candidate_tower, m.candidate_features)):
        h = tower_in(tower, feats)
        for w, b in tower.dense.params():
            h = torch.relu(h @ w.detach().double() + b.detach().double())
        outs.append(h)
    s = outs[0] @ outs[1].t() - m.candidate_logq(x).double()[None, :]
    return float((torch.logsumexp(s, 1) - s.diagonal()).sum())


def _flat_problem(m, x):
    """The history table's flat sparse problem from the model's own last_grad."""
    layer = m.query_tower.input_layer
    off = dict(zip([f.name for f in layer.categorical_features], layer.column_offsets()))["hist"]
    ids = x["hist"].cpu().numpy()
    rows = layer.embedding_layers["hist"].num_rows
    scale = bag_ref.bag_scale(bag_ref.valid_slots(ids, rows).sum(1), "mean")
    g = layer.last_grad.cpu().numpy()[:, off:off + 8]
    ids_flat, G, _ = bag_ref.expand(ids, rows, g, scale, "mean")
    return ids_flat, G


def test_eager_step_loss_and_history_table(cuda):
    m = _model(cuda, 1)
    x = _batch(cuda, np.random.default_rng(2), B)
    assert (x["hist"] == -1).all(1).any() and m.get_input_signature()["hist"].shape == (None, L)
    want = _fp64_loss(m, x)
    table = m.query_tower.input_layer.embedding_layers["hist"]
    before = table.weight.cpu().numpy().copy()
    loss = float(m.train_step(x)["loss"])
    print(f"\nbag model: loss {loss:.6f}, fp64 {want:.6f}, rel {abs(loss - want) / abs(want):.2e}")
    assert abs(loss - want) <= 1e-3 * abs(want)
    ids_flat, G = _flat_problem(m, x)
    ref_t, ref_a = before.copy(), np.full_like(before, 0.1)
    oracle.sparse_adagrad(ref_t, ref_a, ids_flat, G, 0.05, 1e-7)
    assert not np.array_equal(ref_t, before)
    assert np.array_equal(table.weight.cpu().numpy().view(np.int32), ref_t.view(np.int32))
    acc = m.optimizer._slot(table.weight, 1, 0.1)[0]
    assert np.array_equal(acc.cpu().numpy().view(np.int32), ref_a.view(np.int32))
    m.check_optimizer_status()


def test_fused_optimizer_apply_equals_default(cuda):
    a, b = _model(cuda, 3), _model(cuda, 3, fused_optimizer_apply=True)
    rng = np.random.default_rng(4)
    for i in range(3):
        x = _batch(cuda, rng, B)
        la, lb = a.train_step(x)["loss"], b.train_step(x)["loss"]
        assert torch.isfinite(la) and torch.equal(la, lb), i
        _assert_same_state(a, b, i)
    a.check_optimizer_status()
    b.check_optimizer_status()


@pytest.mark.parametrize("optimizer", ["adagrad", "adam"])
def test_tower_with_only_a_sequence_feature(cuda, optimizer):
    """No one-id feature on the query side: no regular sparse call for that
    tower, the bag update still runs (default and fused apply alike)."""
    def build(**kw):
        qf, cf = _features(pooling="sqrtn")
        m = TwoTowerModel(qf[1:], cf, "art", E, [H], [H], device=cuda, seed=17, **kw)
        m.compile(optimizer=OptimizerFactory.get_optimizer(optimizer, {"learning_rate": 0.05}))
        return m

    a, b = build(), build(fused_optimizer_apply=True)
    assert a.query_tower.input_layer.sparse_sources() == [] and a.query_tower.input_layer.output_dim == 8
    rng = np.random.default_rng(18)
    before = a.query_tower.input_layer.embedding_layers["hist"].weight.clone()
    for i in range(2):
        x = _batch(cuda, rng, 65)
        x.pop("cust")
        la, lb = a.train_step(x)["loss"], b.train_step(x)["loss"]
        assert torch.isfinite(la) and torch.equal(la, lb), i
        assert len(a.query_tower.input_layer.bag_sources()) == 1
    for ta, tb in zip(a.towers, b.towers):
        assert torch.equal(ta.dense.flat, tb.dense.flat)
        for n, layer in ta.input_layer.embedding_layers.items():
            assert torch.equal(layer.weight, tb.input_layer.embedding_layers[n].weight), n
    assert not torch.equal(a.query_tower.input_layer.embedding_layers["hist"].weight, before)
    a.check_optimizer_status()
    b.check_optimizer_status()


def test_graphed_step_equals_eager(cuda):
    a, b = _model(cuda, 5), _model(cuda, 5)
    rng = np.random.default_rng(6)
    g = None
    for i in range(3):
        x = _batch(cuda, rng, B)
        la = a.train_step(x)["loss"].clone()
        if g is None:
            g = GraphedTrainStep(b, x, warmup=1)
            lb = g.warmup_out["loss"].clone()
            assert g.static["hist"].shape == (B, L) and g.static["hist"].stride() == (1, B)
        else:
            lb = g(x)["loss"].clone()
        assert torch.equal(la, lb), i
    torch.cuda.synchronize()
    _assert_same_state(a, b)
    b.check_optimizer_status()


def test_graphed_device_fit_equals_eager_host_fit(cuda):
    cols = _columns(np.random.default_rng(7), 100)  # 3 full batches of 32 + a partial one
    a, b = _model(cuda, 8), _model(cuda, 8)
    ha = a.fit(EncodedDataset(cols, 32, 40, seed=9, device=cuda), epochs=2, use_graph=False)
    dev = DeviceDataset(cols, 32, 40, seed=9, device=cuda)
    first = next(iter(DeviceDataset(cols, 32, device=cuda)))
    assert first["hist"].shape == (32, L) and torch.equal(first["hist"], torch.as_tensor(cols["hist"][:32], device=cuda))
    hb = b.fit(dev, epochs=2, use_graph=True)
    torch.cuda.synchronize()
    assert b._device_fit_graph is not None
    np.testing.assert_allclose(hb["loss"], ha["loss"], rtol=1e-12)
    _assert_same_state(a, b)


def test_adam_step(cuda):
    m = _model(cuda, 10, optimizer="adam")
    x = _batch(cuda, np.random.default_rng(11), B)
    table = m.query_tower.input_layer.embedding_layers["hist"]
    before = table.weight.cpu().numpy().copy()
    m.train_step(x)
    ids_flat, G = _flat_problem(m, x)
    ref, mm, vv = before.copy(), np.zeros_like(before), np.zeros_like(before)
    oracle.sparse_adam(ref, mm, vv, ids_flat, G, 1e-3, 0.9, 0.999, 1e-7, 1)
    assert not np.array_equal(ref, before)
    np.testing.assert_allclose(table.weight.cpu().numpy(), ref, rtol=2e-6, atol=1e-7)


def _raw_queries(rng, n):
    hist = [[str(v) for v in rng.integers(0, HV + 10, rng.integers(0, 9))] for _ in range(n)]
    hist[0], hist[1] = [], None
    return {"cust": [str(v) for v in rng.integers(0, 320, n)], "hist": hist}


def test_export_and_retriever_on_list_valued_queries(cuda, tmp_path):
    m = _model(cuda, 12)
    rng = np.random.default_rng(13)
    for _ in range(2):
        m.train_step(_batch(cuda, rng, B))
    raw = _raw_queries(rng, 64)
    enc = m.query_tower.input_layer.encode(raw)
    assert enc["hist"].shape == (64, L) and enc["hist"].dtype == torch.int32
    qe = m.query_tower(enc)
    assert torch.equal(qe, m.query_tower(raw))  # raw nested strings go through encode
    m.save(str(tmp_path / "model") + "/")
    r = TwoTowerModel.load(str(tmp_path / "model") + "/", device=cuda)
    hist = next(f for f in r.query_features if f.name == "hist")
    assert (hist.sequence_length, hist.pooling) == (L, "mean")
    assert torch.equal(r.query_tower(raw), qe)

    cand = {"art": torch.arange(0, 301, dtype=torch.int32, device=cuda),
            "ptn": torch.as_tensor(np.arange(301) % 21, dtype=torch.int32, device=cuda)}
    ids = np.array([f"article-{i}" for i in range(301)])
    index = BruteForceIndex(10, m.query_tower, [(ids, m.candidate_tower(cand))])
    s, idx = index.search(qe)
    index.save(str(tmp_path / "index" / "i"))
    served = Retriever.load(str(tmp_path / "index" / "i"), device=cuda)
    got, scores = served(raw, scores=True)
    assert np.array_equal(got, index.lookup_identifiers(idx)) and torch.equal(scores, s)


def test_model_without_a_sequence_feature_launches_nothing_new(cuda, monkeypatch):
    calls = {"gather_bag": 0, "bag_grad_expand": 0}

    def counted(name):
        fn = getattr(hip_ops, name)

        def wrapper(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapper

    for name in calls:
        monkeypatch.setattr(hip_ops, name, counted(name))
    rng = np.random.default_rng(14)
    for kw in (dict(), dict(fused_optimizer_apply=True), dict(optimizer="adam")):
        plain = _model(cuda, 15, history=False, **kw)
        plain.train_step(_batch(cuda, rng, B, history=False))
        plain.query_tower(_batch(cuda, rng, 7, history=False))
    assert calls == {"gather_bag": 0, "bag_grad_expand": 0}
    m = _model(cuda, 15)
    m.train_step(_batch(cuda, rng, B))
    assert calls == {"gather_bag": 1, "bag_grad_expand": 1}  # one launch each per step
