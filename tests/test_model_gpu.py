"""GPU: the reference-API mirror end to end through libtt.

- the reference's own test vectors through our classes on the GPU
  (BruteForceIndex: tests/test_indices.py; LogQCorrection: test_layers.py;
  IndexRecall with a GPU index);
- full train steps against the numpy fp32 restatement (oracle.CpuTwoTower),
  including the duplicated feature name of main.py;
- hipGraph replay == eager;
- the C3 shape (B=16384, E=128) in-batch passes against a torch fp64
  reference of the same op (row blocks);
- modelling_runner end to end on a tiny encoded dataset.
Tolerances: loss rel 1e-3 (north star); first-step parameter updates rel
1e-2 (bf16 MFMA operands in the loss gradients); index ids bit-exact.
"""
import json
import os

import numpy as np
import pytest
import torch

from oracle import oracle
from pkg import dtypes
from pkg.modelling import hip_ops
from pkg.modelling.indices.brute_force import BruteForceIndex
from pkg.modelling.layers.logq_correction import LogQCorrection
from pkg.modelling.metrics.index_recall import IndexRecall
from pkg.modelling.models.two_tower_model import GraphedTrainStep, TwoTowerModel
from pkg.modelling.optimizer_factory import OptimizerFactory
from pkg.schema.features import Feature, FeatureFamily

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_tests.json")))


def test_bruteforce_index_reference_golden(cuda):
    g = GOLD["bruteforce"]
    vocab = Feature("id", dtypes.string, FeatureFamily.QUERY, embedding_size=2, vocab=g["query_vocab"])
    table = torch.tensor(g["query_embeddings"], device=cuda)

    def mock_query_model(x):  # MockEmbeddingModel of test_indices.py:8-60
        rows = torch.as_tensor(vocab.encode(x["id"]), device=cuda).long()
        return table[rows]

    pairs = [([cid], torch.tensor([emb])) for cid, emb in zip(g["candidate_ids"], g["candidate_embeddings"])]
    index = BruteForceIndex(g["k"], mock_query_model, pairs, device=cuda)
    out = index({"id": np.array(g["queries"]).reshape(-1, 1)})
    assert out.tolist() == g["expected"]
    s, i = index.search(mock_query_model({"id": g["queries"]}))
    assert i.cpu().tolist() == g["derived_topk_indices"]
    assert s.cpu().tolist() == g["derived_topk_scores"]


def test_logq_layer_golden_on_gpu(cuda):
    g = GOLD["logq"]
    out = LogQCorrection(g["candidate_prob_lookup"])(torch.tensor(g["logits"], device=cuda), g["candidate_ids"])
    assert np.array_equal(np.round(out.cpu().numpy(), 5), np.round(np.asarray(g["expected"], np.float32), 5))


def test_index_recall_with_gpu_index(cuda):
    rng = np.random.default_rng(0)
    C = np.maximum(rng.standard_normal((500, 16)), 0).astype(np.float32)
    Q = np.maximum(rng.standard_normal((300, 16)), 0).astype(np.float32)
    true = rng.integers(0, 500, 300).astype(np.int32)
    ids = torch.arange(500, dtype=torch.int32, device=cuda) + 7
    index = BruteForceIndex(20, lambda x: x["q"], [(ids, torch.as_tensor(C))], device=cuda)
    rec = IndexRecall(index, [1, 5, 20])
    ref = oracle.RecallAccumulator([1, 5, 20])
    for s in range(0, 300, 128):
        qb = torch.as_tensor(Q[s:s + 128], device=cuda)
        rec({"q": qb}, torch.as_tensor(true[s:s + 128] + 7, device=cuda))
        _, ri, _ = oracle.bruteforce_topk(Q[s:s + 128], C, 20)
        ref.update(true[s:s + 128] + 7, ri + 7)
    assert rec.metric == ref.metric
    assert all(isinstance(v, np.float64) for v in rec.metric.values())


def _t(x, cuda):
    return torch.as_tensor(x, device=cuda)


def _small_model(cuda, seed=0, logq=True, fused=False, hidden=(64,)):
    V = [str(i) for i in range(300)]
    qf = [Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=16, vocab=V),
          Feature("post", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V[:50])]
    cf = [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=16, vocab=V),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=V[:20]),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=4, vocab=V[:20])]
    rng = np.random.default_rng(seed)
    probs = {str(i): float(p) for i, p in enumerate(rng.dirichlet(np.ones(300)))} if logq else None
    m = TwoTowerModel(qf, cf, "art", 32, list(hidden), list(hidden), probs, device=cuda, seed=seed,
                      fused_optimizer_apply=fused)
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", {"learning_rate": 0.05}))
    return m


def _batch(cuda, rng, B, zipf=True):
    if zipf:
        z = lambda v: torch.as_tensor((rng.zipf(1.3, B) % v).astype(np.int32), device=cuda)
    else:
        z = lambda v: torch.as_tensor(rng.integers(0, v, B).astype(np.int32), device=cuda)
    return {"cust": z(301), "post": z(51), "art": z(301), "ptn": z(21)}


def _cpu_mirror(m, inbatch="fp32"):
    def tables(layer):
        return [layer.embedding_layers[f.name].weight.cpu().numpy().copy() for f in layer.categorical_features]

    def dense(t):
        return [(w.detach().cpu().numpy(), b.detach().cpu().numpy()) for w, b in t.dense.params()]

    ref = oracle.CpuTwoTower(tables(m.query_tower.input_layer), tables(m.candidate_tower.input_layer),
                             dense(m.query_tower), dense(m.candidate_tower), 0.05, inbatch=inbatch)
    # the duplicated name shares ONE table: alias the objects so both lookups update it
    ref.c_tables[2] = ref.c_tables[1]
    ref.c_acc[2] = ref.c_acc[1]
    return ref


@pytest.mark.parametrize("zipf", [True, False])
def test_train_steps_match_cpu_restatement(cuda, zipf):
    """First step: every parameter update within a norm-relative bound of the
    fp32 CPU restatement — 3e-3 for the embedding tables, 1e-2 for the tower
    MLP buffers.  The only non-fp32-faithful arithmetic is the fused loss's
    bf16 MFMA operands (~1e-3 per-example gradient error); the MLP weight
    gradients sum that error over the whole batch, where the exact sum
    largely cancels (P - I), so their relative error is the larger one.
    Observed (round 3, both id distributions): tables <= 2.7e-3, MLP
    buffers <= 6.2e-3.  Then the loss trajectory over 3
    steps within 1e-3 rel (parameters themselves drift apart: lr 0.05 on a
    0.1 accumulator moves embeddings by about their own scale every step, so
    any rounding difference is amplified).  Every tower GEMM is libtt's
    (tt_mlp_rows forward / input gradients, tt_mlp_wgrad weight gradients)."""
    m = _small_model(cuda)
    ref = _cpu_mirror(m)
    rng = np.random.default_rng(5)

    def snapshot():
        ci = m.candidate_tower.input_layer.embedding_layers
        qi = m.query_tower.input_layer.embedding_layers
        return {"art": ci["art"].weight.cpu().numpy().copy(), "ptn": ci["ptn"].weight.cpu().numpy().copy(),
                "cust": qi["cust"].weight.cpu().numpy().copy(), "post": qi["post"].weight.cpu().numpy().copy(),
                "qmlp": m.query_tower.dense.flat.detach().cpu().numpy().copy(),
                "cmlp": m.candidate_tower.dense.flat.detach().cpu().numpy().copy()}

    def ref_snapshot():
        flat = lambda layers: np.concatenate([np.concatenate([w.reshape(-1), b]) for w, b in layers])
        return {"art": ref.c_tables[0], "ptn": ref.c_tables[1], "cust": ref.q_tables[0], "post": ref.q_tables[1],
                "qmlp": flat(ref.q_layers), "cmlp": flat(ref.c_layers)}

    con = _cpu_mirror(m, inbatch="bf16")  # the kernels' arithmetic contract
    before = snapshot()
    for step in range(3):
        b = _batch(cuda, rng, 512, zipf)
        lq = m.candidate_logq(b).cpu().numpy()
        ids = ([b["cust"].cpu().numpy(), b["post"].cpu().numpy()],
               [b["art"].cpu().numpy(), b["ptn"].cpu().numpy(), b["ptn"].cpu().numpy()])
        rl = ref.step(*ids, lq)
        if step == 0:
            con.step(*ids, lq)
        gl = float(m.train_step(b)["loss"].item())
        assert abs(gl - rl) <= 1e-3 * abs(rl), (step, gl, rl)
        if step == 0:
            after, r = snapshot(), ref_snapshot()
            rc = {"art": con.c_tables[0], "ptn": con.c_tables[1], "cust": con.q_tables[0], "post": con.q_tables[1],
                  "qmlp": np.concatenate([np.concatenate([w.reshape(-1), bb]) for w, bb in con.q_layers]),
                  "cmlp": np.concatenate([np.concatenate([w.reshape(-1), bb]) for w, bb in con.c_layers])}
            for k in after:  # includes the shared ptn table (one combined update of both lookups)
                d_gpu, d_ref, d_con = after[k] - before[k], r[k] - before[k], rc[k] - before[k]
                err = np.linalg.norm(d_gpu - d_ref) / np.linalg.norm(d_ref)
                err_c = np.linalg.norm(d_gpu - d_con) / np.linalg.norm(d_con)
                print(f"first-step update {k}: rel err {err:.2e} (fp32), {err_c:.2e} (contract)")
                assert err <= (1e-2 if k.endswith("mlp") else 3e-3), (k, err)
                assert err_c <= 2e-3, (k, err_c)


@pytest.mark.parametrize("B", [1, 2, 37, 1000])
def test_ragged_batch_train_step_matches_cpu_restatement(cuda, B):
    """Batch sizes off every tile multiple (the reference's last partial batch,
    tfrecord_dataset.py:97 has no drop_remainder), including B = 1 (the loss
    of a one-column softmax is 0 in exact arithmetic; here lse comes from the
    bf16-MFMA score and the positive logit from the fp32 one, so it is 0 to
    within the bf16 rounding of that score: atol 1e-4, far above the certified
    bound of a score of this model's magnitude)."""
    m = _small_model(cuda, seed=B)
    ref = _cpu_mirror(m)
    rng = np.random.default_rng(B)
    b = _batch(cuda, rng, B, True)
    lq = m.candidate_logq(b).cpu().numpy()
    rl = ref.step([b["cust"].cpu().numpy(), b["post"].cpu().numpy()],
                  [b["art"].cpu().numpy(), b["ptn"].cpu().numpy(), b["ptn"].cpu().numpy()], lq)
    gl = float(m.train_step(b)["loss"].item())
    assert np.isfinite(gl)
    assert abs(gl - rl) <= 1e-3 * abs(rl) + 1e-4, (gl, rl)


def _state(m):
    out = {}
    for t, name in ((m.query_tower, "q"), (m.candidate_tower, "c")):
        out[name + ".mlp"] = t.dense.flat.detach().clone()
        out[name + ".mlp_acc"] = m.optimizer._slot(t.dense.flat, 1, 0.1)[0].clone()
        for n, layer in t.input_layer.embedding_layers.items():
            out[f"{name}.{n}"] = layer.weight.detach().clone()
            out[f"{name}.{n}.acc"] = m.optimizer._slot(layer.weight, 1, 0.1)[0].clone()
    return out


def test_fused_optimizer_apply_bit_identical_to_unfused(cuda):
    """fused_optimizer_apply (each tower's dense + sparse Adagrad applied inside
    the backward, on the tower's stream and workspace scope) gives bit-identical
    tables, accumulators and MLP buffers to the unfused step, at ragged batch
    sizes that change between steps (stale presorted workspaces of another
    size must be detected, never read); the first step also matches the CPU
    restatement; no sparse error is recorded (tt_sparse_status)."""
    a, b = _small_model(cuda, seed=11), _small_model(cuda, seed=11, fused=True)
    ref = _cpu_mirror(b)
    rng = np.random.default_rng(9)
    for i, B in enumerate((512, 37, 256, 1, 300)):
        x = _batch(cuda, rng, B, True)
        la = a.train_step(x)["loss"]
        lb = b.train_step(x)["loss"]
        if i == 0:
            lq = b.candidate_logq(x).cpu().numpy()
            rl = ref.step([x["cust"].cpu().numpy(), x["post"].cpu().numpy()],
                          [x["art"].cpu().numpy(), x["ptn"].cpu().numpy(), x["ptn"].cpu().numpy()], lq)
            assert abs(float(lb) - rl) <= 1e-3 * abs(rl)
            r = ref.c_tables[0]
            got = b.candidate_tower.input_layer.embedding_layers["art"].weight.cpu().numpy()
            before = _small_model(cuda, seed=11).candidate_tower.input_layer.embedding_layers["art"].weight
            d_ref, d_gpu = r - before.cpu().numpy(), got - before.cpu().numpy()
            assert np.linalg.norm(d_gpu - d_ref) <= 1e-2 * np.linalg.norm(d_ref)
        assert torch.equal(la, lb), (i, B)
        sa, sb = _state(a), _state(b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (i, B, k)
        # the fused step leaves nothing for a later apply_gradients to re-apply
        assert all(t.dense.flat.grad is None and t.input_layer.last_grad is None for t in b.towers)
    a.optimizer.check_status(cuda)
    b.optimizer.check_status(cuda)


@pytest.mark.parametrize("fused", [False, True])
def test_igrad_first_order_bit_identical(cuda, monkeypatch, fused):
    """TT_IGRAD_FIRST (off by default): each tower's input-gradient chain before
    its weight gradients, and in the fused step the embedding update issued at
    the input gradient, ahead of the weight gradients on that tower's stream —
    the same kernels on the same operands, so losses, tables, accumulators and
    MLP buffers stay bit-identical to the layer-by-layer order, step for step
    at ragged batch sizes; no sparse error is recorded."""
    from pkg.modelling.models import tower as tower_mod

    a, b = _small_model(cuda, seed=12, fused=fused), _small_model(cuda, seed=12, fused=fused)
    rng = np.random.default_rng(10)
    for i, B in enumerate((512, 37, 256, 300)):
        x = _batch(cuda, rng, B, True)
        monkeypatch.setattr(tower_mod, "IGRAD_FIRST", False)
        la = a.train_step(x)["loss"]
        monkeypatch.setattr(tower_mod, "IGRAD_FIRST", True)
        lb = b.train_step(x)["loss"]
        assert torch.equal(la, lb), (i, B)
        sa, sb = _state(a), _state(b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (i, B, k)
    a.optimizer.check_status(cuda)
    b.optimizer.check_status(cuda)


def test_dense_early_bit_identical_to_dense_after_join(cuda, monkeypatch):
    """The default step applies each tower's dense (MLP) Adagrad inside the
    backward on the tower's stream (TT_DENSE_EARLY); with it off the dense
    step runs after the join.  Tables, accumulators, MLP buffers and losses
    are bit-identical at ragged batch sizes, and apply_gradients is left with
    only the embedding update (no dense update applied twice)."""
    from pkg.modelling.models import two_tower_model as ttm

    a, b = _small_model(cuda, seed=5), _small_model(cuda, seed=5)
    rng = np.random.default_rng(4)
    for i, B in enumerate((512, 37, 256, 1)):
        x = _batch(cuda, rng, B, True)
        monkeypatch.setattr(ttm, "DENSE_EARLY", False)
        la = a.train_step(x)["loss"]
        monkeypatch.setattr(ttm, "DENSE_EARLY", True)
        lb = b.train_step(x)["loss"]
        # both towers' dense updates were applied inside the backward, and nothing is left to re-apply
        assert b.last_step.mode == "dense_early" and b.last_step.dense_done == {0, 1}
        assert a.last_step.mode == "plain" and a.last_step.dense_done == set()
        assert all(t.dense.flat.grad is None for t in b.towers)
        assert torch.equal(la, lb), (i, B)
        sa, sb = _state(a), _state(b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (i, B, k)
    a.optimizer.check_status(cuda)
    b.optimizer.check_status(cuda)


@pytest.mark.parametrize("fused", [False, True])
def test_paired_tower_launches_bit_identical(cuda, monkeypatch, fused):
    """TT_TOWER_PAIR (both towers' MLP layers as paired launches on one
    stream: tt_mlp_rows_pair / tt_mlp_wgrad_pair) gives bit-identical losses,
    tables, accumulators and MLP buffers to the two-stream step, unfused and
    with the fused optimizer apply, at ragged batch sizes."""
    from pkg.modelling import losses

    a, b = _small_model(cuda, seed=21, fused=fused), _small_model(cuda, seed=21, fused=fused)
    rng = np.random.default_rng(6)
    for i, B in enumerate((512, 37, 256, 1)):
        x = _batch(cuda, rng, B, True)
        monkeypatch.setattr(losses, "TOWER_PAIR", 0)
        la = a.train_step(x)["loss"]
        monkeypatch.setattr(losses, "TOWER_PAIR", 1)
        lb = b.train_step(x)["loss"]
        assert torch.equal(la, lb), (i, B)
        sa, sb = _state(a), _state(b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (i, B, k)
    a.optimizer.check_status(cuda)
    b.optimizer.check_status(cuda)


@pytest.mark.parametrize("pair", [0, 1])
def test_fused_dense_wgrad_bit_identical(cuda, monkeypatch, pair):
    """TT_FUSED_DENSE_WGRAD: each layer's Adagrad step applied by its
    weight-gradient launches (tt_mlp_wgrad_adagrad) instead of one
    dense_adagrad launch per tower gives bit-identical losses, tables,
    accumulators and MLP buffers at ragged batch sizes (and, with paired
    tower launches, falls back to the dense launch)."""
    from pkg.modelling import losses
    from pkg.modelling.models import two_tower_model as ttm

    monkeypatch.setattr(losses, "TOWER_PAIR", pair)
    a, b = _small_model(cuda, seed=41), _small_model(cuda, seed=41)
    rng = np.random.default_rng(14)
    for i, B in enumerate((512, 37, 256, 1)):
        x = _batch(cuda, rng, B, True)
        monkeypatch.setattr(ttm, "FUSED_DENSE_WGRAD", False)
        la = a.train_step(x)["loss"]
        monkeypatch.setattr(ttm, "FUSED_DENSE_WGRAD", True)
        lb = b.train_step(x)["loss"]
        assert all(bool(ts.fused_layers) == (pair == 0) for ts in b.last_step.towers)
        assert torch.equal(la, lb), (i, B)
        sa, sb = _state(a), _state(b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (i, B, k)
    a.optimizer.check_status(cuda)
    b.optimizer.check_status(cuda)


@pytest.mark.parametrize("pair", [0, 1])
def test_pack_with_gather_bit_identical(cuda, monkeypatch, pair):
    """TT_PACK_WITH_GATHER: the towers' MLP weight images packed by the train
    step's gather launch (tt_gather_multi_pack) instead of one pack launch
    per tower: bit-identical losses, tables, accumulators and MLP buffers at
    ragged batch sizes, eager and graphed (and with paired tower launches)."""
    from pkg.modelling import losses
    from pkg.modelling.models import two_tower_model as ttm

    monkeypatch.setattr(losses, "TOWER_PAIR", pair)
    a, b = _small_model(cuda, seed=43), _small_model(cuda, seed=43)
    rng = np.random.default_rng(15)
    for i, B in enumerate((512, 37, 256, 1)):
        x = _batch(cuda, rng, B, True)
        monkeypatch.setattr(ttm, "PACK_WITH_GATHER", False)
        la = a.train_step(x)["loss"]
        monkeypatch.setattr(ttm, "PACK_WITH_GATHER", True)
        lb = b.train_step(x)["loss"]
        # packed by the gather launch with the flag on, by each tower's forward with it off
        assert all(ts.packed for ts in b.last_step.towers) and not any(ts.packed for ts in a.last_step.towers)
        assert torch.equal(la, lb), (i, B)
        sa, sb = _state(a), _state(b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (i, B, k)
    batches = [_batch(cuda, rng, 256, True) for _ in range(4)]
    ga = GraphedTrainStep(a, batches[0], warmup=1)
    monkeypatch.setattr(ttm, "PACK_WITH_GATHER", False)
    gb = GraphedTrainStep(b, batches[0], warmup=1)
    for x in batches[1:]:
        assert torch.equal(ga(x)["loss"], gb(x)["loss"])
    torch.cuda.synchronize()
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_fused_dense_wgrad_odd_hidden_width_bit_identical(cuda, monkeypatch):
    """A hidden width that is not a multiple of 4 (towers [68, 66] -> 32: the
    66-wide layer runs tt_mlp_wgrad on padded copies) leaves the next layer's
    region of the flat buffer 8-B aligned: TT_FUSED_DENSE_WGRAD applies the
    aligned layers' Adagrad in their weight-gradient launches and leaves that
    layer to the dense step (DenseStack._layer_adagrad) — losses, tables,
    accumulators and MLP buffers bit-identical to the dense step for every
    layer, at ragged batch sizes (tt_mlp_wgrad_adagrad used to refuse the
    unaligned region and fail the step)."""
    from pkg.modelling.models import two_tower_model as ttm

    a, b = _small_model(cuda, seed=49, hidden=(68, 66)), _small_model(cuda, seed=49, hidden=(68, 66))
    rng = np.random.default_rng(17)
    for i, B in enumerate((512, 37, 256, 1)):
        x = _batch(cuda, rng, B, True)
        monkeypatch.setattr(ttm, "FUSED_DENSE_WGRAD", False)
        la = a.train_step(x)["loss"]
        monkeypatch.setattr(ttm, "FUSED_DENSE_WGRAD", True)
        lb = b.train_step(x)["loss"]
        # layer 0 applied by its weight-gradient launch; layer 1 (width 66, padded path) and
        # layer 2 (its region 8-B aligned) by the dense step
        assert all(ts.fused_layers == {0} for ts in b.last_step.towers)
        assert torch.equal(la, lb), (i, B)
        sa, sb = _state(a), _state(b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (i, B, k)
    a.optimizer.check_status(cuda)
    b.optimizer.check_status(cuda)


def test_gather_multi_pack_equals_two_launches(cuda):
    """tt_gather_multi_pack: the gather and the weight images of one launch
    equal tt_gather_multi + tt_mlp_pack_many, byte for byte."""
    from pkg.modelling.models.tower import DenseStack

    g = torch.Generator()
    g.manual_seed(3)
    st = DenseStack(37, [66, 128], cuda, g)
    rng = np.random.default_rng(8)
    B = 1000
    tab = torch.as_tensor(rng.standard_normal((500, 32)).astype(np.float32), device=cuda)
    ids = _t(rng.integers(-2, 505, B).astype(np.int32), cuda)
    num = torch.as_tensor(rng.standard_normal(B).astype(np.float32), device=cuda)
    outs = [torch.full((B, 36), 7.0, device=cuda) for _ in range(2)]
    flat = st.flat.detach()
    jobs = st.prepack_jobs(flat)
    hip_ops.gather_multi([([(num, None, 0), (tab, ids, 1)], outs[0])], B, pack_jobs=jobs)
    imgs1 = {k: v.clone() for k, v in st.images.items()}
    for v in st.images.values():
        v.zero_()
    hip_ops.gather_multi([([(num, None, 0), (tab, ids, 1)], outs[1])], B)
    hip_ops.mlp_pack_many(jobs)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    for k, v in st.images.items():
        assert torch.equal(v, imgs1[k]), k


@pytest.mark.parametrize("fused", [False, True])
def test_split_prep_bit_identical(cuda, monkeypatch, fused):
    """TT_SPLIT_PREP (each tower's bf16 loss operand prepared on its own
    stream, then tt_inbatch_softmax_xent_prepped) gives bit-identical losses,
    tables, accumulators and MLP buffers to the one-call loss entry, unfused
    and with the fused optimizer apply, at ragged batch sizes."""
    from pkg.modelling import losses

    a, b = _small_model(cuda, seed=23, fused=fused), _small_model(cuda, seed=23, fused=fused)
    rng = np.random.default_rng(8)
    for i, B in enumerate((512, 37, 256, 1)):
        x = _batch(cuda, rng, B, True)
        monkeypatch.setattr(losses, "SPLIT_PREP", False)
        la = a.train_step(x)["loss"]
        monkeypatch.setattr(losses, "SPLIT_PREP", True)
        lb = b.train_step(x)["loss"]
        assert torch.equal(la, lb), (i, B)
        sa, sb = _state(a), _state(b)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (i, B, k)
    a.optimizer.check_status(cuda)
    b.optimizer.check_status(cuda)


def test_stale_presorted_workspace_is_reported_not_applied(cuda):
    """A presorted sparse apply whose workspace holds another call's sorted
    keys applies nothing and is reported by tt_sparse_status (TTError), the
    table left untouched; a matching apply afterwards reports nothing."""
    from pkg._native import TTError

    rng = np.random.default_rng(2)
    V, D, B = 1000, 16, 512
    t = torch.as_tensor(rng.uniform(-0.05, 0.05, (V, D)).astype(np.float32), device=cuda)
    acc = torch.full_like(t, 0.1)
    ids_a = torch.as_tensor(rng.integers(0, V, B).astype(np.int32), device=cuda)
    ids_b = torch.as_tensor(rng.integers(0, V, B).astype(np.int32), device=cuda)
    g = torch.as_tensor(rng.standard_normal((B, D)).astype(np.float32), device=cuda)
    spec = lambda ids: [dict(table=t, slot0=acc, ids=[ids], grad_col_offset=[0], grad=g)]
    with hip_ops.Workspace.scope("stale_test"):
        hip_ops.sparse_sort(spec(ids_a), B)
        before = t.clone()
        hip_ops.sparse_adagrad(spec(ids_b), B, None, 0.05, 1e-7, presorted=True)  # keys are ids_a's
        with pytest.raises(TTError, match="another call"):
            hip_ops.sparse_status(cuda, "sparse")
        assert torch.equal(t, before)
        hip_ops.sparse_sort(spec(ids_b), B)
        hip_ops.sparse_adagrad(spec(ids_b), B, None, 0.05, 1e-7, presorted=True)
        hip_ops.sparse_status(cuda, "sparse")
        assert not torch.equal(t, before)


def test_graph_replay_equals_eager(cuda):
    a, b = _small_model(cuda, seed=3), _small_model(cuda, seed=3)
    rng = np.random.default_rng(1)
    batches = [_batch(cuda, rng, 256) for _ in range(4)]
    for x in batches:
        a.train_step(x)
    g = GraphedTrainStep(b, batches[0], warmup=1)
    for x in batches[1:]:
        g(x)
    torch.cuda.synchronize()
    for ta, tb in zip(a.towers, b.towers):
        assert torch.equal(ta.dense.flat, tb.dense.flat)
        for n in ta.input_layer.embedding_layers:
            assert torch.equal(ta.input_layer.embedding_layers[n].weight, tb.input_layer.embedding_layers[n].weight)


def test_graph_replays_back_to_back_equal_eager(cuda):
    """40 replays of the captured train step queued back to back (one sync at
    the end, as bench.py and fit run them) leave the state bit-identical to
    40 eager steps: a replay never overlaps the previous one, whose freed
    and re-used temporaries the next replay's first nodes would otherwise
    clobber."""
    a, b = _small_model(cuda, seed=8), _small_model(cuda, seed=8)
    rng = np.random.default_rng(21)
    batches = [_batch(cuda, rng, 4096) for _ in range(41)]
    for x in batches:
        a.train_step(x)
    g = GraphedTrainStep(b, batches[0], warmup=1)
    packed = [g.pack(x) for x in batches[1:]]
    torch.cuda.synchronize()
    for p in packed:
        g(packed=p)
    torch.cuda.synchronize()
    for ta, tb in zip(a.towers, b.towers):
        assert torch.equal(ta.dense.flat, tb.dense.flat)
        for n in ta.input_layer.embedding_layers:
            assert torch.equal(ta.input_layer.embedding_layers[n].weight, tb.input_layer.embedding_layers[n].weight)


def test_c3_shape_inbatch_passes_vs_torch_fp64(cuda):
    """Full C3 size (B=16384, E=128): rows/cols passes against a torch fp64
    reference evaluated in row blocks on the GPU."""
    B, E = 16384, 128
    g = torch.Generator(device=cuda)
    g.manual_seed(0)
    q = torch.relu(torch.randn(B, E, generator=g, device=cuda)) * 0.15
    c = torch.relu(torch.randn(B, E, generator=g, device=cuda)) * 0.15
    logq = torch.log(torch.rand(B, generator=g, device=cuda) * 1e-3 + 1e-6)
    lse, row_loss, dq = hip_ops.inbatch_rows(q, c, logq)
    dc = hip_ops.inbatch_cols(q, lse, c, logq)
    qd, cd, ld = q.double(), c.double(), logq.double()
    dc_ref = torch.zeros_like(cd)
    loss_ref = 0.0
    err_dq = 0.0
    nrm_dq = 0.0
    for s in range(0, B, 2048):
        S = qd[s:s + 2048] @ cd.T - ld[None, :]
        lse_ref = torch.logsumexp(S, 1)
        r = torch.arange(s, min(s + 2048, B), device=cuda)
        loss_ref += float((lse_ref - S[r - s, r]).sum())
        P = torch.exp(S - lse_ref[:, None])
        P[r - s, r] -= 1.0
        dq_ref = P @ cd
        err_dq += float(((dq[s:s + 2048].double() - dq_ref) ** 2).sum())
        nrm_dq += float((dq_ref ** 2).sum())
        dc_ref += P.T @ qd[s:s + 2048]
        assert torch.allclose(lse[s:s + 2048].double(), lse_ref, rtol=1e-3, atol=1e-3)
    loss = float(row_loss.double().sum())
    assert abs(loss - loss_ref) <= 1e-3 * abs(loss_ref)
    assert (err_dq / nrm_dq) ** 0.5 <= 1e-2
    assert float(torch.linalg.norm(dc.double() - dc_ref) / torch.linalg.norm(dc_ref)) <= 1e-2


def test_modelling_runner_end_to_end(cuda, tmp_path):
    import pandas as pd

    from pkg.modelling.dataset import EncodedDataset, encode_dataframe
    from pkg.modelling.runner import modelling_runner
    from pkg.schema.model_config import ModelConfig
    from pkg.schema.schema import Schema
    from pkg.schema.training_config import TrainingConfig
    from pkg.utils.settings import Settings

    rng = np.random.default_rng(0)
    n = 3000
    df = pd.DataFrame({"customer_id": rng.integers(0, 200, n).astype(str),
                       "article_id": (rng.zipf(1.3, n) % 400).astype(str),
                       "section": rng.integers(0, 7, n).astype(str)})
    feats = [Feature("customer_id", dtypes.string, FeatureFamily.QUERY, embedding_size=16),
             Feature("article_id", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=16),
             Feature("section", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=4)]
    schema = Schema(feats, TrainingConfig(256, 512, "adagrad", {"learning_rate": 0.05}, candidate_batch_size=128,
                                          epochs=2), ModelConfig(16, [1, 10, 50], [32], [32]))
    train, test = df.iloc[:2500], df.iloc[2500:]
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
    model = modelling_runner(s)
    assert os.path.exists(f"{d}/model/two_tower.pt") and os.path.exists(f"{d}/index/i.pt")
    sd = torch.load(f"{d}/model/two_tower.pt", weights_only=True)
    assert "query_tower.dense.flat" in sd


def test_sharded_train_step_world1_matches_single_gpu(cuda):
    """ShardedTrainStep on a 1-rank RCCL group (large tables sharded, small
    ones replicated with dense all-reduced gradients) is bit-identical to the
    single-GPU train step: same summation orders, same Adagrad arithmetic."""
    import socket

    import torch.distributed as dist

    from pkg.modelling.distributed import destroy_process_group
    from pkg.modelling.distributed import ShardedTrainStep

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device(cuda))
    try:
        a, b = _small_model(cuda, seed=3), _small_model(cuda, seed=3)
        step = ShardedTrainStep(a, shard_min_rows=300, global_negatives=False)
        assert step.tables is not None and len(step.tables.names) == 2
        rng = np.random.default_rng(7)
        batches = [_batch(cuda, rng, 256) for _ in range(5)]
        # call 1 eager, then the captured middle; routing prefetched from call 3 on
        for i, batch in enumerate(batches):
            nxt = batches[i + 1] if 2 <= i + 1 < len(batches) else None
            la = step(batch, next_batch=nxt)["loss"]
            lb = b.train_step(batch)["loss"]
            assert torch.equal(la, lb), i
        for ta, tb in zip(a.towers, b.towers):
            assert torch.equal(ta.dense.flat, tb.dense.flat)
            for name, t in tb.input_layer.embedding_layers.items():
                mine = ta.input_layer.embedding_layers[name]
                full = step.tables.gather_full(mine._shard_key) if hasattr(mine, "_shard_key") else mine.weight
                assert torch.equal(full, t.weight), name
    finally:
        destroy_process_group()  # the captured step graphs first, then the group


@pytest.mark.parametrize("B", [256, 4096])
def test_global_negatives_step_captures_rccl_collectives(cuda, monkeypatch, B):
    """ShardedTrainStep's global-negatives middle with its collectives as real
    RCCL calls (a one-rank process group with BatchComm(always=True), so the
    all_gathers / reduce_scatters run even at world 1) captured into the
    step's hipGraph — the default over RCCL — trains bit-identically to the
    same step run eagerly (TT_SHARDED_EAGER=1), step for step.  At 4096 rows
    per rank (losses.GLOBAL_TOWER_STREAMS) the towers' two-stream fork/join is
    captured together with the collectives."""
    import socket

    import torch.distributed as dist

    from pkg.modelling.distributed import destroy_process_group
    from pkg.modelling.distributed import BatchComm, ShardedTrainStep

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device(cuda))
    try:
        a, b = _small_model(cuda, seed=5), _small_model(cuda, seed=5)
        graphed = ShardedTrainStep(a, shard_min_rows=300, global_negatives=True, comm=BatchComm(always=True))
        monkeypatch.setenv("TT_SHARDED_EAGER", "1")
        eager = ShardedTrainStep(b, shard_min_rows=300, global_negatives=True, comm=BatchComm(always=True))
        monkeypatch.delenv("TT_SHARDED_EAGER")
        assert graphed.use_graph and not eager.use_graph
        from pkg.modelling import losses

        assert (B >= losses.GLOBAL_TOWER_STREAMS) == (B == 4096)
        rng = np.random.default_rng(9)
        batches = [_batch(cuda, rng, B) for _ in range(5)]
        for i, batch in enumerate(batches):  # call 1 eager, then graph replays
            la, lb = graphed(batch)["loss"], eager(batch)["loss"]
            assert torch.equal(la, lb), i
        assert graphed._graph is not None
        for ta, tb in zip(a.towers, b.towers):
            assert torch.equal(ta.dense.flat, tb.dense.flat)
            for name, t in tb.input_layer.embedding_layers.items():
                mine = ta.input_layer.embedding_layers[name]
                ga = graphed.tables.gather_full(mine._shard_key) if hasattr(mine, "_shard_key") else mine.weight
                gb = eager.tables.gather_full(t._shard_key) if hasattr(t, "_shard_key") else t.weight
                assert torch.equal(ga, gb), name
        graphed.check_status()
        eager.check_status()
    finally:
        destroy_process_group()  # the captured step graphs first, then the group


@pytest.mark.parametrize("B", [2048, 16384])
def test_sharded_step_routed_exchanges_captured_on_rccl(cuda, monkeypatch, B):
    """The N > 1 step's structure on one GPU over RCCL: ShardedTrainStep(
    global_negatives=True, always_exchange=True) on a one-rank RCCL group runs
    the routed exchanges — the requests', rows' and per-request gradients'
    all_to_alls and the bucket's all_reduce — as real collectives inside the
    step's captured hipGraph (at world 1 they are otherwise skipped).  For 5
    steps (call 1 eager, then replays) it trains bit-identically to the
    world-1 shortcut step and to the single-GPU GraphedTrainStep; the status
    words and the overflow canary stay clean."""
    import socket

    import torch.distributed as dist

    from pkg.modelling.distributed import ShardedTrainStep, destroy_process_group

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device(cuda))
    try:
        a, b, c = (_small_model(cuda, seed=8) for _ in range(3))
        xchg = ShardedTrainStep(a, shard_min_rows=300, global_negatives=True, always_exchange=True)
        short = ShardedTrainStep(b, shard_min_rows=300, global_negatives=True)
        assert xchg.use_graph and xchg.exchange and not short.exchange and xchg.tables is not None
        rng = np.random.default_rng(B)
        batches = [_batch(cuda, rng, B) for _ in range(5)]
        single = GraphedTrainStep(c, batches[0], warmup=1)  # its warm-up step trains on batch 0
        for i, batch in enumerate(batches):
            la, lb = xchg(batch)["loss"], short(batch)["loss"]
            lc = single.warmup_out["loss"] if i == 0 else single(batch)["loss"]
            assert torch.equal(la, lb) and torch.equal(la, lc), (i, la, lb, lc)
        assert xchg._graph is not None and short._graph is not None
        torch.cuda.synchronize()
        assert xchg._canary.tolist() == [0x7EADBEEF, 0, 0x7EADBEEF]
        for ta, tb, tc in zip(a.towers, b.towers, c.towers):
            assert torch.equal(ta.dense.flat, tb.dense.flat) and torch.equal(ta.dense.flat, tc.dense.flat)
            for name, t in tc.input_layer.embedding_layers.items():
                ma, mb = ta.input_layer.embedding_layers[name], tb.input_layer.embedding_layers[name]
                ga = xchg.tables.gather_full(ma._shard_key) if hasattr(ma, "_shard_key") else ma.weight
                gb = short.tables.gather_full(mb._shard_key) if hasattr(mb, "_shard_key") else mb.weight
                assert torch.equal(ga, gb) and torch.equal(ga, t.weight), name
        xchg.check_status()
        short.check_status()
    finally:
        destroy_process_group()  # the captured step graphs first, then the group


def test_sharded_step_status_reports_stale_owner_keys(cuda):
    """ShardedTrainStep.check_status reads the workspaces the sharded step's
    sparse kernels write ("sparse_owner": the owners' Adagrad apply,
    "sparse_mid": the per-request sums): a presorted owner apply that finds
    another call's sorted keys there applies nothing and check_status raises
    (the reference's legacy apply raises too, optimizer_factory.py:15-18);
    the check clears it, so a second check is quiet."""
    import socket

    import torch.distributed as dist

    from pkg.modelling.distributed import destroy_process_group
    from pkg._native import TTError
    from pkg.modelling.distributed import ShardedTrainStep

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        m = _small_model(cuda, seed=6)
        step = ShardedTrainStep(m, shard_min_rows=300, global_negatives=True)
        rng = np.random.default_rng(4)
        for _ in range(2):
            step(_batch(cuda, rng, 256))
        step.check_status()  # a clean run: nothing recorded
        name = step.tables.names[0]
        t, acc = step.tables.shard[name], step.tables.acc[name]
        B, D = 128, t.shape[1]
        ids_a = torch.as_tensor(rng.integers(0, t.shape[0], B).astype(np.int32), device=cuda)
        ids_b = torch.as_tensor(rng.integers(0, t.shape[0], B).astype(np.int32), device=cuda)
        g = torch.ones(B, D, dtype=torch.float32, device=cuda)
        spec = lambda ids: [dict(table=t, slot0=acc, ids=[ids], grad_col_offset=[0], grad=g)]
        before = t.clone()
        hip_ops.sparse_sort(spec(ids_a), B, ws_tag="sparse_owner")
        hip_ops.sparse_adagrad(spec(ids_b), B, None, 0.05, 1e-7, presorted=True, ws_tag="sparse_owner")
        with pytest.raises(TTError, match="another call"):
            step.check_status()
        assert torch.equal(t, before)
        step.check_status()
    finally:
        destroy_process_group()  # the captured step graphs first, then the group


def test_model_call_score_matrix_on_libtt(cuda):
    """TwoTowerModel.call without gradients (the reference's public score
    matrix, two_tower_model.py:65-92) comes from hip_ops.score_matrix (bf16x3
    tt_mlp_rows over 256-candidate chunks): within 2e-5 of the fp64 product of
    the same tower outputs, at a ragged candidate count."""
    m = _small_model(cuda, seed=31)
    rng = np.random.default_rng(12)
    x = _batch(cuda, rng, 601, True)
    with torch.no_grad():
        s = m.call(x, training=False)
        q, c = m._split(x)
        qe, ce = m.query_tower.call(q), m.candidate_tower.call(c)
    ref = qe.double() @ ce.double().t()
    assert s.shape == (601, 601)
    err = (s.double() - ref).abs().max().item() / ref.abs().max().item()
    assert err <= 2e-5, err
    # odd embedding width (padded to 16-B rows inside)
    a = torch.rand(37, 13, device=cuda)
    b = torch.rand(300, 13, device=cuda)
    r = hip_ops.score_matrix(a, b)
    assert torch.allclose(r.double(), a.double() @ b.double().t(), rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("nq,nc,e", [(601, 601, 64), (37, 517, 13), (300, 5, 130)])
def test_score_matrix_autograd_on_libtt(cuda, nq, nc, e):
    """hip_ops.ScoreMatrix (TwoTowerModel.call with gradients): S = q.c^T and
    its gradients dq = G.c, dc = G^T.q all on tt_mlp_rows (bf16x3, K and N
    chunked by 256, partials added in chunk order) — within 2e-5 (relative to
    the largest entry) of the fp64 autograd product, ragged and odd sizes
    included; deterministic."""
    g0 = torch.Generator(device=cuda)
    g0.manual_seed(nq + nc + e)
    q = torch.randn(nq, e, device=cuda, generator=g0).requires_grad_()
    c = torch.randn(nc, e, device=cuda, generator=g0).requires_grad_()
    w = torch.randn(nq, nc, device=cuda, generator=g0)
    s = hip_ops.ScoreMatrix.apply(q, c)
    (s * w).sum().backward()
    q64, c64 = q.detach().double().requires_grad_(), c.detach().double().requires_grad_()
    s64 = q64 @ c64.t()
    (s64 * w.double()).sum().backward()
    for got, ref in ((s, s64), (q.grad, q64.grad), (c.grad, c64.grad)):
        err = (got.detach().double() - ref.detach()).abs().max().item() / ref.detach().abs().max().item()
        assert err <= 2e-5, err
    dq1 = q.grad.clone()
    q.grad = None
    hip_ops.ScoreMatrix.apply(q, c).mul(w).sum().backward()
    assert torch.equal(q.grad, dq1)


def test_model_call_with_gradients_on_libtt(cuda):
    """TwoTowerModel.call with gradients enabled differentiates through the
    libtt score matrix (no torch.matmul): the towers' flat MLP gradients of
    sum(S * W) within 1e-4 (relative norm) of the same towers with the
    product taken by a torch fp32 matmul (the test's reference only)."""
    m = _small_model(cuda, seed=32)
    rng = np.random.default_rng(13)
    x = _batch(cuda, rng, 300, True)
    w = torch.randn(300, 300, device=cuda, generator=torch.Generator(device=cuda).manual_seed(5))
    flats = [t.dense.flat for t in m.towers]
    for f in flats:
        f.grad = None
    s = m.call(x, training=True)
    assert s.requires_grad and "ScoreMatrix" in type(s.grad_fn).__name__
    (s * w).sum().backward()
    got = [f.grad.clone() for f in flats]
    for f in flats:
        f.grad = None
    q, c = m._split(x)
    qe, ce = m.query_tower.call(q), m.candidate_tower.call(c)
    ((qe @ ce.t()) * w).sum().backward()
    for g, f in zip(got, flats):
        assert torch.isfinite(g).all()
        err = ((g - f.grad).norm() / f.grad.norm()).item()
        assert err <= 1e-4, err


@pytest.mark.parametrize("variant", ["nested_join", "sibling_join", "origin_join"])
def test_capture_guard_refuses_nested_joins(cuda, variant):
    """hip_ops.capture_guard checks the capture's fork / join structure as it
    is issued: a side branch waiting on the sub-branch it forked
    (tools/graph_fork_probe.py nested_join, which crashes ROCm 7.2's
    hipStreamEndCapture) or on a sibling branch raises NestedJoinError before
    that wait is issued, and the capture still ends cleanly; the origin
    joining every branch (origin_join) captures and replays correctly."""
    x = torch.arange(1 << 16, dtype=torch.float32, device=cuda)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    out = {}

    def body():
        cur = torch.cuda.current_stream()
        s1.wait_stream(cur)
        if variant == "sibling_join":
            s2.wait_stream(cur)
        with torch.cuda.stream(s1):
            y = x * 2
            if variant != "sibling_join":
                s2.wait_stream(s1)  # a fork from a branch: legal
        with torch.cuda.stream(s2):
            z = (y if variant != "sibling_join" else x) + 1
        if variant == "origin_join":
            cur.wait_stream(s1)
            cur.wait_stream(s2)
            out["w"] = y * 3 + z
        else:
            s1.wait_stream(s2)  # a branch joining a branch: refused
            with torch.cuda.stream(s1):
                w = z * 3
            cur.wait_stream(s1)
            out["w"] = w

    body()  # eager: any order is fine outside a capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    if variant == "origin_join":
        with hip_ops.capture_guard([]), torch.cuda.graph(g, capture_error_mode="thread_local"):
            body()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["w"], x * 2 * 3 + x * 2 + 1)
    else:
        with pytest.raises(hip_ops.NestedJoinError, match="origin"):
            with hip_ops.capture_guard([]), torch.cuda.graph(g, capture_error_mode="thread_local"):
                body()
        torch.cuda.synchronize()  # the refused capture ended cleanly: the device is usable
        assert torch.equal(x * 2, torch.arange(1 << 16, dtype=torch.float32, device=cuda) * 2)
