"""GPU: cosine scoring (normalize_embeddings / temperature) through the public
interface — the loss node's composition, fp64 accuracy under TT_INBATCH_X3=1,
equivalent configurations, graphed / sharded training and serving.

Common shape: B = 96 (not a multiple of 64), E = 32, one hidden layer of 48,
small vocabularies, logQ on."""
import numpy as np
import pytest
import torch

from pkg import dtypes
from pkg.modelling import hip_ops
from pkg.modelling.indices.brute_force import BruteForceIndex
from pkg.modelling.models.tower import Tower
from pkg.modelling.models.two_tower_model import GraphedTrainStep, TwoTowerModel
from pkg.modelling.optimizer_factory import OptimizerFactory
from pkg.schema.features import Feature, FeatureFamily

pytestmark = pytest.mark.gpu

T = 0.05
B, E, H = 96, 32, 48


def _model(cuda, seed=0, **kw):
    V = [str(i) for i in range(300)]
    qf = [Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=16, vocab=V),
          Feature("post", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V[:50])]
    cf = [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=16, vocab=V),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=V[:20])]
    rng = np.random.default_rng(seed)
    probs = {str(i): float(p) for i, p in enumerate(rng.dirichlet(np.ones(300)))}
    m = TwoTowerModel(qf, cf, "art", E, [H], [H], probs, device=cuda, seed=seed, **kw)
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", {"learning_rate": 0.05}))
    return m


def _batch(cuda, rng, n, duplicates=False):
    z = lambda v: torch.as_tensor(rng.integers(0, v, n).astype(np.int32), device=cuda)
    x = {"cust": z(301), "post": z(51), "art": z(301), "ptn": z(21)}
    if duplicates:  # the same article several times in the batch
        x["art"][n // 2:] = x["art"][:n - n // 2]
        x["art"][5:9] = x["art"][4]
    return x


def _inputs(m, x):
    """The gathered tower inputs of batch x as fresh leaves, its logQ and ids."""
    q, c = m._split(x)
    with torch.no_grad():
        qi = m.query_tower.input_layer(q).clone()
        ci = m.candidate_tower.input_layer(c).clone()
    return qi, ci, m.candidate_logq(x), m.candidate_ids(x)


def _model_grads(m, x):
    """(loss, d flat_q, d flat_c, d qi, d ci) of the model's fused loss node."""
    qi, ci, logq, ids = _inputs(m, x)
    qi.requires_grad_(True)
    ci.requires_grad_(True)
    for t in m.towers:
        t.dense.flat.grad = None
    loss = m.tower_loss(qi, ci, logq, ids)
    loss.backward()
    torch.cuda.synchronize()
    out = (loss.detach().clone(), m.query_tower.dense.flat.grad.clone(), m.candidate_tower.dense.flat.grad.clone(),
           qi.grad.clone(), ci.grad.clone())
    for t in m.towers:
        t.dense.flat.grad = None
    return out


def _hand_grads(m, x, x3):
    """The same step assembled by hand: forward_acts, l2norm_rows,
    inbatch_fused, l2norm_rows_grad (in place), backward_acts."""
    qi, ci, logq, ids = _inputs(m, x)
    sq, sc = m.query_tower.dense, m.candidate_tower.dense
    fq, fc = sq.flat.detach(), sc.flat.detach()
    ca = sc.forward_acts(ci, fc)
    qa = sq.forward_acts(qi, fq)
    (qn, iq), (cn, ic) = hip_ops.l2norm_rows([(qa[-1], 1.0 / T), (ca[-1], 1.0)])
    _, _, dq, dc, loss = hip_ops.inbatch_fused(qn, cn, logq, loss_scale=1.0, x3=x3, ids=ids)
    hip_ops.l2norm_rows_grad([(qa[-1], iq, dq, 1.0 / T, dq), (ca[-1], ic, dc, 1.0, dc)])
    one = torch.ones(1, dtype=torch.float32, device=qi.device)
    gci, gfc = sc.backward_acts(ca, fc, dc, one, True)
    gqi, gfq = sq.backward_acts(qa, fq, dq, one, True)
    torch.cuda.synchronize()
    return loss, gfq, gfc, gqi, gci


NAMES = ("loss", "d flat_q", "d flat_c", "d qi", "d ci")


@pytest.mark.parametrize("variant", ["default", "x3", "hits"])
def test_loss_node_is_the_hand_assembled_chain(cuda, monkeypatch, variant):
    if variant == "x3":
        monkeypatch.setenv("TT_INBATCH_X3", "1")
    m = _model(cuda, 1, normalize_embeddings=True, temperature=T, remove_accidental_hits=variant == "hits")
    x = _batch(cuda, np.random.default_rng(2), B, duplicates=variant == "hits")
    if variant == "hits":
        assert len(torch.unique(x["art"])) < B // 2 + 8
    got = _model_grads(m, x)
    want = _hand_grads(m, x, x3=variant == "x3")
    assert torch.isfinite(got[0]) and got[1].abs().max() > 0 and got[4].abs().max() > 0
    for name, g, w in zip(NAMES, got, want):
        assert torch.equal(g, w), (variant, name)


def _fp64_chain(m, x):
    """torch fp64 autograd of the whole chain: towers, normalise (zero rows
    stay zero and get no gradient), / T, logQ, CE-SUM with eye labels."""
    qi, ci, logq, _ = _inputs(m, x)
    leaves, outs = [], []
    for t, inp in ((m.query_tower, qi), (m.candidate_tower, ci)):
        h = inp.double().requires_grad_(True)
        params = [(w.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True))
                  for w, b in t.dense.params()]
        leaves.append((h, params))
        for w, b in params:
            h = torch.relu(h @ w + b)
        ss = (h * h).sum(1, keepdim=True)
        live = ss > 0
        inv = torch.where(live, torch.where(live, ss, torch.ones_like(ss)).rsqrt(), torch.zeros_like(ss))
        outs.append(h * inv * t.output_scale)
    s = outs[0] @ outs[1].t() - logq.double()[None, :]
    loss = (torch.logsumexp(s, 1) - s.diagonal()).sum()
    loss.backward()
    flats = [torch.cat([torch.cat([w.grad.reshape(-1), b.grad]) for w, b in params]) for _, params in leaves]
    return loss.detach(), flats[0], flats[1], leaves[0][0].grad, leaves[1][0].grad


def test_x3_chain_against_fp64(cuda, monkeypatch):
    """The project's standing x3 tolerances: loss 1e-4 relative, every
    gradient within 1e-3 of the reference's largest magnitude."""
    monkeypatch.setenv("TT_INBATCH_X3", "1")
    m = _model(cuda, 3, normalize_embeddings=True, temperature=T)
    x = _batch(cuda, np.random.default_rng(4), B)
    got = _model_grads(m, x)
    want = _fp64_chain(m, x)
    assert m.query_tower.output_scale == 1.0 / T
    rel = abs(got[0].double().item() - want[0].item()) / abs(want[0].item())
    print(f"\ncosine x3 vs fp64: loss rel {rel:.3e}")
    errs = []
    for name, g, w in zip(NAMES[1:], got[1:], want[1:]):
        e = ((g.double() - w).abs().max() / w.abs().max()).item()
        print(f"  {name}: max err / max |ref| = {e:.3e}  (max |ref| {w.abs().max().item():.3e})")
        errs.append((name, e))
    assert rel <= 1e-4, rel
    for name, e in errs:
        assert e <= 1e-3, (name, e)


def test_no_temperature_equals_temperature_one(cuda):
    a = _model(cuda, 5, normalize_embeddings=True)
    b = _model(cuda, 5, normalize_embeddings=True, temperature=1.0)
    x = _batch(cuda, np.random.default_rng(6), B)
    for name, ga, gb in zip(NAMES, _model_grads(a, x), _model_grads(b, x)):
        assert torch.equal(ga, gb), name


def test_feature_off_equals_model_without_the_keywords(cuda):
    a = _model(cuda, 7, normalize_embeddings=False, temperature=None)
    b = _model(cuda, 7)
    x = _batch(cuda, np.random.default_rng(8), B)
    for name, ga, gb in zip(NAMES, _model_grads(a, x), _model_grads(b, x)):
        assert torch.equal(ga, gb), name
    for _ in range(2):
        assert torch.equal(a.train_step(x)["loss"], b.train_step(x)["loss"])
    for ta, tb in zip(a.towers, b.towers):
        assert torch.equal(ta.dense.flat, tb.dense.flat)
    # ... and differs from the feature on (the option does something)
    c = _model(cuda, 7, normalize_embeddings=True, temperature=T)
    assert not torch.equal(_model_grads(c, x)[0], _model_grads(b, x)[0])


class _OneRankAlways:
    """A one-rank comm that still runs the global-negatives step's rows /
    columns entries (what every rank runs at G > 1), without a process group."""
    world, rank, always = 1, 0, True

    @staticmethod
    def all_gather(t):
        return t.clone()


def test_rows_cols_entries_are_the_hand_assembled_chain(cuda):
    """global_towers_inbatch_softmax_xent on the rows / cols entries: one
    l2norm_rows launch before them, one in-place l2norm_rows_grad after."""
    from pkg.modelling.losses import global_towers_inbatch_softmax_xent

    m = _model(cuda, 13, normalize_embeddings=True, temperature=T)
    x = _batch(cuda, np.random.default_rng(14), B)
    qi, ci, logq, _ = _inputs(m, x)
    sq, sc = m.query_tower.dense, m.candidate_tower.dense
    qi.requires_grad_(True)
    ci.requires_grad_(True)
    loss = global_towers_inbatch_softmax_xent(qi, ci, sq, sc, _OneRankAlways(), logq)
    loss.backward()
    got = (loss.detach(), sq.flat.grad.clone(), sc.flat.grad.clone(), qi.grad, ci.grad)
    sq.flat.grad = sc.flat.grad = None

    qj, cj = qi.detach(), ci.detach()
    fq, fc = sq.flat.detach(), sc.flat.detach()
    ca, qa = sc.forward_acts(cj, fc), sq.forward_acts(qj, fq)
    (qn, iq), (cn, ic) = hip_ops.l2norm_rows([(qa[-1], 1.0 / T), (ca[-1], 1.0)])
    lse, row_loss, dq = hip_ops.inbatch_rows(qn, cn, logq)
    dc = hip_ops.inbatch_cols(qn, lse, cn, logq, row_loss=row_loss)
    hip_ops.l2norm_rows_grad([(qa[-1], iq, dq, 1.0 / T, dq), (ca[-1], ic, dc, 1.0, dc)])
    one = torch.ones(1, dtype=torch.float32, device=cuda)
    gci, gfc = sc.backward_acts(ca, fc, dc, one, True)
    gqi, gfq = sq.backward_acts(qa, fq, dq, one, True)
    want = (hip_ops.loss_sum(row_loss, 1.0), gfq, gfc, gqi, gci)
    for name, g, w in zip(NAMES, got, want):
        assert torch.equal(g, w), name


@pytest.mark.parametrize("path", ["paired_towers", "fused_optimizer_apply", "both"])
def test_other_step_forms_train_bit_identically(cuda, monkeypatch, path):
    """The paired-launch towers (TT_TOWER_PAIR) and the fused optimizer apply
    under cosine scoring: the same losses and state as the plain cosine step."""
    from pkg.modelling import losses
    from test_model_gpu import _state

    kw = dict(normalize_embeddings=True, temperature=T)
    a = _model(cuda, 15, **kw)
    b = _model(cuda, 15, fused_optimizer_apply=path != "paired_towers", **kw)
    rng = np.random.default_rng(16)
    for i, n in enumerate((256, 37, B)):
        x = _batch(cuda, rng, n)
        monkeypatch.setattr(losses, "TOWER_PAIR", 0)
        la = a.train_step(x)["loss"]
        monkeypatch.setattr(losses, "TOWER_PAIR", 0 if path == "fused_optimizer_apply" else 1)
        lb = b.train_step(x)["loss"]
        assert torch.isfinite(la) and torch.equal(la, lb), (i, n)
        sa, sb = _state(a), _state(b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (i, n, k)
    a.optimizer.check_status(cuda)
    b.optimizer.check_status(cuda)


def _same_state(a, b, tables=None):
    for ta, tb in zip(a.towers, b.towers):
        assert torch.equal(ta.dense.flat, tb.dense.flat)
        for name, t in tb.input_layer.embedding_layers.items():
            mine = ta.input_layer.embedding_layers[name]
            full = tables.gather_full(mine._shard_key) if hasattr(mine, "_shard_key") else mine.weight
            assert torch.equal(full, t.weight), name


@pytest.fixture(scope="module")
def trained(cuda):
    """Three steps at B = 256 with cosine scoring at T = 0.05: eagerly, as a
    GraphedTrainStep (warm-up step, capture, two replays) and as the world-1
    ShardedTrainStep with global negatives (call 1 eager, call 2 captures and
    replays, call 3 replays).  Returns the three models, their losses and
    the sharded step's tables."""
    import socket

    import torch.distributed as dist

    from pkg.modelling.distributed import ShardedTrainStep, destroy_process_group

    kw = dict(normalize_embeddings=True, temperature=T)
    eager, graphed, sharded = (_model(cuda, 9, **kw) for _ in range(3))
    rng = np.random.default_rng(10)
    batches = [_batch(cuda, rng, 256) for _ in range(3)]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device(cuda))
    try:
        step = ShardedTrainStep(sharded, shard_min_rows=300, global_negatives=True)
        assert step.use_graph and step.tables is not None
        losses = []
        g = None
        for i, x in enumerate(batches):
            le = eager.train_step(x)["loss"].clone()
            if i == 0:
                g = GraphedTrainStep(graphed, x, warmup=1)
                lg = g.warmup_out["loss"].clone()
            else:
                lg = g(x)["loss"].clone()
            ls = step(x)["loss"].clone()
            losses.append((le, lg, ls))
        torch.cuda.synchronize()
        assert step._graph is not None
        step.check_status()
        full = {}
        for t in sharded.towers:
            for name, layer in t.input_layer.embedding_layers.items():
                if hasattr(layer, "_shard_key"):
                    full[name] = step.tables.gather_full(layer._shard_key).clone()
                else:
                    full[name] = layer.weight.detach().clone()
        flats = [t.dense.flat.detach().clone() for t in sharded.towers]
    finally:
        destroy_process_group()  # the captured step graph first, then the group
    return dict(eager=eager, graphed=graphed, losses=losses, sharded_tables=full, sharded_flats=flats)


def test_graphed_step_equals_eager(trained):
    for i, (le, lg, _) in enumerate(trained["losses"]):
        assert torch.isfinite(le) and torch.equal(le, lg), i
    _same_state(trained["graphed"], trained["eager"])


def test_world1_sharded_step_equals_eager(trained):
    for i, (le, _, ls) in enumerate(trained["losses"]):
        assert torch.equal(le, ls), i
    for t, flat in zip(trained["eager"].towers, trained["sharded_flats"]):
        assert torch.equal(t.dense.flat, flat)
        for name, layer in t.input_layer.embedding_layers.items():
            assert torch.equal(layer.weight, trained["sharded_tables"][name]), name


def _candidates(cuda):
    return {"art": torch.arange(0, 301, dtype=torch.int32, device=cuda),
            "ptn": torch.as_tensor(np.arange(301) % 21, dtype=torch.int32, device=cuda)}


def test_serving_scores_are_cosine_over_temperature(cuda, trained, tmp_path):
    from pkg.modelling.export import Retriever

    m = trained["eager"]
    cand = m.candidate_tower(_candidates(cuda))
    norms = cand.double().norm(dim=1)
    dead = (cand == 0).all(dim=1)
    assert torch.all((norms[~dead] - 1.0).abs() <= 2e-6) and torch.all(norms[dead] == 0)
    assert (~dead).sum() > 200

    rng = np.random.default_rng(11)
    raw = {"cust": [str(v) for v in rng.integers(0, 320, 64)], "post": [str(v) for v in rng.integers(0, 60, 64)]}
    enc = m.query_tower.input_layer.encode(raw)
    qe = m.query_tower(enc)
    qn = qe.double().norm(dim=1)
    assert torch.all(((qn - 1.0 / T).abs() <= 2e-6 / T) | (qn == 0))
    ids = np.array([f"article-{i}" for i in range(301)])
    index = BruteForceIndex(10, m.query_tower, [(ids, cand)])
    s, idx = index.search(qe)
    ref = (qe.double() @ cand.double().t()).gather(1, idx.long())
    assert torch.all((s.double() - ref).abs() <= 1e-5 * ref.abs())
    assert s.min() >= 0 and s.max() <= (1.0 / T) * (1 + 1e-5)
    assert s.max() > 1.0  # cos / T, not cos

    # Tower.save / load: bit-identical outputs
    m.query_tower.save(str(tmp_path / "q.pt"))
    m.candidate_tower.save(str(tmp_path / "c.pt"))
    rq, rc = Tower.load(str(tmp_path / "q.pt"), cuda), Tower.load(str(tmp_path / "c.pt"), cuda)
    assert (rq.normalize, rq.output_scale, rc.normalize, rc.output_scale) == (True, 1.0 / T, True, 1.0)
    assert torch.equal(rq(enc), qe) and torch.equal(rc(_candidates(cuda)), cand)
    # the whole model
    m.save(str(tmp_path / "model") + "/")
    r = TwoTowerModel.load(str(tmp_path / "model") + "/", device=cuda)
    assert (r.normalize_embeddings, r.temperature) == (True, T)
    assert torch.equal(r.query_tower(enc), qe) and torch.equal(r.candidate_tower(_candidates(cuda)), cand)

    # save_index -> Retriever.load: bit-identical ids and scores
    index.save(str(tmp_path / "index" / "i"))
    served = Retriever.load(str(tmp_path / "index" / "i"), device=cuda)
    got, scores = served(raw, scores=True)
    assert np.array_equal(got, index.lookup_identifiers(idx)) and torch.equal(scores, s)


def test_call_returns_training_logits_before_logq(cuda, trained):
    m = trained["eager"]
    x = _batch(cuda, np.random.default_rng(12), B)
    with torch.no_grad():
        s = m.call(x, training=False)
    q, c = m._split(x)
    ref = m.query_tower(q).double() @ m.candidate_tower(c).double().t()
    assert s.shape == (B, B) and torch.all((s.double() - ref).abs() <= 1e-5 * (1.0 / T))
    assert s.min() >= 0 and s.max() <= (1.0 / T) * (1 + 1e-5)
    # the evaluation loss (no gradients; both outputs normalised in one
    # launch) is the loss of the towers' public outputs, bit for bit
    qi, ci, logq, ids = _inputs(m, x)
    with torch.no_grad():
        ev = m.compute_loss(x, training=False)
        want = m.loss(m.query_tower.dense(qi), m.candidate_tower.dense(ci), logq, ids)
    assert torch.isfinite(ev) and torch.equal(ev, want)
