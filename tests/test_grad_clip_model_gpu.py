"""GPU: gradient clipping (clipvalue / clipnorm / global_clipnorm) through
TwoTowerModel.train_step on every form of the step, for Adagrad and Adam.

The small two-tower model of tests/test_model_gpu.py (vocab 300, embedding
sizes 16 / 8 / 4 with a doubled name, hidden 64, joint 32, logQ).
- a clip that never triggers leaves the default step's state bit for bit;
- a triggering clip: the device's sums of squares and factors match the numpy
  restatement (grad_clip_ref) of a twin's gradients within the kernel-level
  bounds of tests/test_grad_clip_gpu.py, and the state equals the twin
  applying its own gradients, clamped and multiplied by the device factors,
  through the unclipped optimizer, bit for bit;
- GraphedTrainStep and the device-resident fit equal the eager clipped run;
- with a sequence feature, mixed negatives, accidental hits and sample
  weights: eager == graphed, sums of squares from the twin's gradients with
  bag rows counted only where valid.
"""
import numpy as np
import pytest
import torch

import grad_clip_ref as ref
from pkg import dtypes
from pkg.modelling.dataset import CandidateCatalogue, DeviceDataset, EncodedDataset
from pkg.modelling.models.two_tower_model import GraphedTrainStep, TwoTowerModel
from pkg.modelling.optimizer_factory import OptimizerFactory
from pkg.schema.features import Feature, FeatureFamily

pytestmark = pytest.mark.gpu

V = [str(i) for i in range(300)]
BATCHES = [512, 37, 1]


def _features(seq=False):
    qf = [Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=16, vocab=V),
          Feature("post", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V[:50])]
    if seq:
        qf.append(Feature("hist", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V[:30],
                          sequence_length=5, pooling="mean"))
    cf = [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=16, vocab=V),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=V[:20]),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=4, vocab=V[:20])]
    return qf, cf


def _model(cuda, opt, clip=None, seed=0, seq=False, **kw):
    qf, cf = _features(seq)
    rng = np.random.default_rng(seed)
    probs = {str(i): float(p) for i, p in enumerate(rng.dirichlet(np.ones(300)))}
    m = TwoTowerModel(qf, cf, "art", 32, [64], [64], probs, device=cuda, seed=seed, **kw)
    m.compile(optimizer=OptimizerFactory.get_optimizer(opt, dict({"learning_rate": 0.05}, **(clip or {}))))
    return m


def _batch(cuda, rng, B, seq=False):
    z = lambda v: torch.as_tensor((rng.zipf(1.3, B) % v).astype(np.int32), device=cuda)  # noqa: E731
    x = {"cust": z(301), "post": z(51), "art": z(301), "ptn": z(21)}
    if seq:
        h = rng.integers(0, 31, (B, 5)).astype(np.int32)
        h[rng.random((B, 5)) < 0.4] = -1  # pads
        h[0] = -1                         # an all-pad row
        if B > 1:
            h[1] = [3, 7, 7, 0, 30]       # a full row
        x["hist"] = torch.as_tensor(h, device=cuda)
    return x


def _state(m):
    """Tables, MLP buffers and every optimizer slot, by name."""
    out = {}
    for t, name in ((m.query_tower, "q"), (m.candidate_tower, "c")):
        params = [("mlp", t.dense.flat)] + [(n, l.weight) for n, l in t.input_layer.embedding_layers.items()]
        for n, p in params:
            out[f"{name}.{n}"] = p.detach().clone()
            for i, s in enumerate(m.optimizer._slots.get(id(p), [])):
                out[f"{name}.{n}.slot{i}"] = s.clone()
    return out


def _assert_same_state(a, b, what):
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (what, k)


def _backward_only(m, x):
    """The step's forward and backward with no update from inside the
    backward (the path a clipping optimizer takes), nothing applied."""
    for t in m.towers:
        t.dense.flat.grad = None
    loss = m.compute_loss(x, training=True)
    loss.backward()
    return loss.detach()


def _twin_variables(m):
    """The twin's gradient values per variable, in plan order, as numpy:
    [(name, [arrays])]; bag rows only where the slot is valid."""
    out = []
    for t, tname in ((m.query_tower, "query"), (m.candidate_tower, "candidate")):
        fg = t.dense.flat.grad.cpu().numpy()
        for li, (w, fi, fo, b) in enumerate(t.dense.layout):
            out.append((f"{tname}/dense_{li}/kernel", [fg[w:w + fi * fo]]))
            out.append((f"{tname}/dense_{li}/bias", [fg[b:b + fo]]))
        layer = t.input_layer
        lg = layer.last_grad.cpu().numpy()
        by_name = {}
        bags = iter(layer.bag_sources())
        for f, off in zip(layer.categorical_features, layer.column_offsets()):
            dim = layer.embedding_layers[f.name].dim
            cols = lg[:, off:off + dim]
            if f.is_sequence:
                bag = next(bags)
                ids, scale = bag["ids"].cpu().numpy(), bag["scale"].cpu().numpy()
                G = np.repeat(cols * scale[:, None], ids.shape[1], axis=0)  # row b * L + l
                ok = ((ids >= 0) & (ids < bag["table"].num_rows)).ravel()
                cols = G[ok]
            by_name.setdefault(f.name, []).append(cols)
        out += [(f"{tname}/embedding/{n}", arrs) for n, arrs in by_name.items()]
    return out


def _check_device_sums(opt, variables, clip):
    """The kernel-level bounds of test_grad_clip_gpu.py on the optimizer's
    monitoring tensors; returns the device factors."""
    assert opt.clip_variable_names == [n for n, _ in variables]
    ss_dev = opt.last_clip_sumsq.cpu().numpy()
    f_dev = opt.last_clip_factors.cpu().numpy()
    cv = clip.get("clipvalue")
    ss_ref = [ref.sumsq(a, cv) for _, a in variables]
    for v, (name, arrs) in enumerate(variables):
        n = sum(a.size for a in arrs)
        assert abs(ss_dev[v] - ss_ref[v]) <= n * 2.0 ** -52 * ss_ref[v], (name, ss_dev[v], ss_ref[v])
    if "clipnorm" in clip:
        for v, (name, _) in enumerate(variables):
            assert f_dev[v].tobytes() in ref.factor_candidates(ss_ref[v], clip["clipnorm"]), (name, f_dev[v])
    else:
        total = ref.sumsq([a for _, arrs in variables for a in arrs], cv)
        assert all(f.tobytes() in ref.factor_candidates(total, clip["global_clipnorm"]) for f in f_dev)
        assert len(set(f_dev.tolist())) == 1
    return f_dev


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("clip", [{"clipvalue": 3e38, "clipnorm": 1e30}, {"global_clipnorm": 1e30}],
                         ids=["value-norm", "global"])
def test_clip_that_never_triggers_is_the_default_step_bitwise(cuda, opt, clip):
    for B in BATCHES:
        rng = np.random.default_rng(20 + B)
        batches = [_batch(cuda, rng, B) for _ in range(3)]
        a, b = _model(cuda, opt, clip, seed=1), _model(cuda, opt, None, seed=1)
        for x in batches:
            assert torch.equal(a.train_step(x)["loss"], b.train_step(x)["loss"]), (B, opt)
        _assert_same_state(a, b, (B, opt))
        assert (a.optimizer.last_clip_factors == 1.0).all()
        assert a.optimizer.iterations == b.optimizer.iterations == 3


# clipnorm = 0.5 after clipvalue = 1e-3 cannot bring a factor below 1 in this
# model: its largest variable has 512 * 16 = 8192 values, so a clamped norm is
# at most 1e-3 * sqrt(8192) = 0.0905.  That case is kept and must show the
# clamp at work (and factors of exactly 1); the third case has both at work.
TRIGGERING = [({"global_clipnorm": 1.0}, "factor"), ({"clipnorm": 0.5, "clipvalue": 1e-3}, "clamp"),
              ({"clipnorm": 0.01, "clipvalue": 1e-3}, "factor")]


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("clip,active", TRIGGERING, ids=["global", "norm-value", "small-norm-value"])
def test_triggering_clip_against_a_twin(cuda, opt, clip, active):
    triggered = []  # batch sizes at which a factor fell below 1
    for B in BATCHES:
        rng = np.random.default_rng(30 + B)
        a, twin = _model(cuda, opt, clip, seed=2), _model(cuda, opt, None, seed=2)
        # two steps: the second meets existing slots and, for Adam, a step count past 0
        for step in range(2):
            x = _batch(cuda, rng, B)
            la = a.train_step(x)["loss"]
            assert torch.equal(la, _backward_only(twin, x))
            variables = _twin_variables(twin)
            f = _check_device_sums(a.optimizer, variables, clip)
            print(f"{opt} {clip} B={B} step {step}: factors {sorted(set(f.tolist()))[:4]}")
            # at B = 1 the in-batch loss is constant (one candidate): a zero gradient, nothing to clip
            if (f < 1.0).any():
                triggered.append(B)
            if B > 1 and active == "clamp":
                assert max(float(np.abs(v).max()) for _, arrs in variables for v in arrs) > clip["clipvalue"]
                assert (f == 1.0).all()
            _apply_scaled(twin, variables, f, clip)
            _assert_same_state(a, twin, (B, opt, step))
    # it did not pass idle (B = 37 stays below a global norm of 1; B = 1 has nothing to clip)
    assert (512 in triggered) if active == "factor" else not triggered


def _apply_scaled(twin, variables, f_dev, clip):
    """The twin's own gradients, clamped and multiplied by the device factors
    with torch, applied through its unclipped optimizer."""
    fac = {name: float(f) for (name, _), f in zip(variables, f_dev)}
    cv = clip.get("clipvalue")

    def scale(g, f):
        if cv is not None:
            g.clamp_(-float(np.float32(cv)), float(np.float32(cv)))
        g.mul_(f)

    for t, tname in ((twin.query_tower, "query"), (twin.candidate_tower, "candidate")):
        fg = t.dense.flat.grad
        for li, (w, fi, fo, b) in enumerate(t.dense.layout):
            scale(fg[w:w + fi * fo], fac[f"{tname}/dense_{li}/kernel"])
            scale(fg[b:b + fo], fac[f"{tname}/dense_{li}/bias"])
        layer = t.input_layer
        for f, off in zip(layer.categorical_features, layer.column_offsets()):
            dim = layer.embedding_layers[f.name].dim
            scale(layer.last_grad[:, off:off + dim], fac[f"{tname}/embedding/{f.name}"])
    twin.optimizer.apply_gradients(twin.towers)


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_graphed_step_equals_eager(cuda, opt):
    clip = {"global_clipnorm": 1.0}
    rng = np.random.default_rng(40)
    batches = [_batch(cuda, rng, 512) for _ in range(5)]
    a, b = _model(cuda, opt, clip, seed=3), _model(cuda, opt, clip, seed=3)
    want = [a.train_step(x)["loss"].clone() for x in batches]
    g = GraphedTrainStep(b, batches[0], warmup=1)  # Adam: on the device clock from here on
    got = [g.warmup_out["loss"].clone()] + [g(x)["loss"].clone() for x in batches[1:]]  # 4 replays
    torch.cuda.synchronize()
    assert g.reusable(b, batch=batches[0])
    for i, (p, q) in enumerate(zip(got, want)):
        assert torch.equal(p, q), (opt, i)
    _assert_same_state(a, b, opt)
    assert float(b.optimizer.last_clip_factors.min()) < 1.0
    assert torch.equal(a.optimizer.last_clip_sumsq, b.optimizer.last_clip_sumsq)
    if opt == "adam":  # the device clock counts the replays
        assert a.optimizer.iterations == b.optimizer.iterations == 5


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_device_resident_fit_equals_eager(cuda, opt):
    clip = {"clipnorm": 0.01, "clipvalue": 1e-3}  # both at work at B = 37
    rng = np.random.default_rng(41)
    B, nb = 37, 3
    batches = [_batch(cuda, rng, B) for _ in range(nb)]
    tail = _batch(cuda, rng, 5)  # the partial last batch runs eagerly
    a, b = _model(cuda, opt, clip, seed=4), _model(cuda, opt, clip, seed=4)
    want = []
    for _ in range(2):
        ls = [a.train_step(x)["loss"].double() for x in batches + [tail]]
        want.append(float(sum(ls).item()) / (nb + 1))
    cols = {k: np.concatenate([x[k].cpu().numpy() for x in batches + [tail]]) for k in batches[0]}
    ds = DeviceDataset.from_encoded(EncodedDataset(cols, batch_size=B, device=cuda))
    hist = b.fit(ds, epochs=2, use_graph=True)
    assert hist["loss"] == want
    _assert_same_state(a, b, opt)
    assert float(b.optimizer.last_clip_factors.min()) < 1.0


def _catalogue(cuda):
    rng = np.random.default_rng(42)
    _, cf = _features()
    cols = {"art": np.arange(1, 201).astype(np.int32), "ptn": rng.integers(0, 21, 200).astype(np.int32)}
    return CandidateCatalogue(cols, cf, device=cuda)


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_composition_with_the_other_options(cuda, opt):
    """A sequence feature (L = 5, mean pooling; pads, an all-pad row, a full
    row), mixed negatives (M = 64: the candidate tower runs B + M rows),
    accidental-hit removal and sample weights under a triggering
    global_clipnorm."""
    clip = {"global_clipnorm": 0.1}
    kw = dict(seq=True, num_sampled_negatives=64, sampled_negatives_seed=5, remove_accidental_hits=True)
    rng = np.random.default_rng(50)
    B = 512
    batches = [_batch(cuda, rng, B, seq=True) for _ in range(3)]
    for x in batches:
        x["__weight__"] = torch.as_tensor(rng.uniform(0.1, 1.0, B).astype(np.float32), device=cuda)
    models = [_model(cuda, opt, c, seed=6, **kw) for c in (clip, clip, None)]
    for m in models:
        m.set_candidate_catalogue(_catalogue(cuda))
        m.sample_weight_scale = 2.0
    a, b, twin = models
    want = [a.train_step(x)["loss"].clone() for x in batches[:1]]
    # the first step against the twin's gradients
    assert torch.equal(_backward_only(twin, batches[0]), want[0])
    assert twin.candidate_tower.input_layer.last_grad.shape[0] == B + 64
    f = _check_device_sums(a.optimizer, _twin_variables(twin), clip)
    assert f[0] < 1.0
    want += [a.train_step(x)["loss"].clone() for x in batches[1:]]
    g = GraphedTrainStep(b, batches[0], warmup=1)
    got = [g.warmup_out["loss"].clone()] + [g(x)["loss"].clone() for x in batches[1:]]
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(got, want)):
        assert torch.equal(p, q), (opt, i)
    _assert_same_state(a, b, opt)
    a.check_optimizer_status()
    b.check_optimizer_status()
