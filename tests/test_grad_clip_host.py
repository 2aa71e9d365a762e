"""CPU: gradient clipping's host side: the optimizer keywords (Keras legacy
clipvalue / clipnorm / global_clipnorm), the region plan, the refusals, the
numpy restatement against a naive loop, and the C entries' argument checks
(nothing is launched by these calls)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import grad_clip_ref as ref
from pkg import _native, dtypes
from pkg.modelling.models.two_tower_model import TwoTowerModel
from pkg.modelling.optimizer_factory import (Adagrad, Adam, OptimizerFactory, clip_tower_desc, plan_clip_regions)
from pkg.schema.features import Feature, FeatureFamily

CPU = torch.device("cpu")
Q, C = FeatureFamily.QUERY, FeatureFamily.CANDIDATE
V = [str(i) for i in range(30)]


@pytest.mark.parametrize("cls", [Adagrad, Adam])
def test_keywords_are_stored(cls):
    o = cls(learning_rate=0.1)
    assert (o.clipvalue, o.clipnorm, o.global_clipnorm, o.clips) == (None, None, None, False)
    o = cls(learning_rate=0.1, clipvalue=0.5, clipnorm=2)
    assert (o.clipvalue, o.clipnorm, o.global_clipnorm, o.clips) == (0.5, 2.0, None, True)
    o = cls(learning_rate=0.1, global_clipnorm=1.0, clipvalue=None, decay=0.0)
    assert (o.clipvalue, o.clipnorm, o.global_clipnorm, o.clips) == (None, None, 1.0, True)
    assert o.last_clip_sumsq is None and o.last_clip_factors is None and o.clip_variable_names == []


@pytest.mark.parametrize("cls", [Adagrad, Adam])
def test_keyword_validation(cls):
    with pytest.raises(ValueError, match="clipnorm.*global_clipnorm"):
        cls(learning_rate=0.1, clipnorm=1.0, global_clipnorm=1.0)
    for key in ("clipvalue", "clipnorm", "global_clipnorm"):
        for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "1", True):
            with pytest.raises(ValueError, match=key):
                cls(learning_rate=0.1, **{key: bad})
    with pytest.raises(TypeError, match="clip_norm"):
        cls(learning_rate=0.1, clip_norm=1.0)


@pytest.mark.parametrize("cls", [Adagrad, Adam])
def test_decay_is_still_refused(cls):
    with pytest.raises(NotImplementedError) as e:
        cls(learning_rate=0.1, decay=1e-3)
    assert "decay" in str(e.value) and "clip" not in str(e.value)
    with pytest.raises(NotImplementedError):
        cls(learning_rate=0.1, decay=1e-3, clipnorm=1.0)


@pytest.mark.parametrize("name", ["adagrad", "adam"])
def test_factory_constructs_a_clipping_optimizer(name):
    o = OptimizerFactory.get_optimizer(name, {"learning_rate": 0.05, "global_clipnorm": 1.0})
    assert o.global_clipnorm == 1.0 and o.clips
    o = OptimizerFactory.get_optimizer(name, {"learning_rate": 0.05, "clipvalue": 0.5, "clipnorm": 0.25})
    assert (o.clipvalue, o.clipnorm) == (0.5, 0.25)


def _model(**kw):
    qf = [Feature("age", dtypes.float32, Q),
          Feature("cust", dtypes.string, Q, embedding_size=8, vocab=V),
          Feature("hist", dtypes.string, Q, embedding_size=4, vocab=V, sequence_length=5)]
    cf = [Feature("art", dtypes.string, C, embedding_size=8, vocab=V),
          Feature("ptn", dtypes.string, C, embedding_size=4, vocab=V[:5]),
          Feature("ptn", dtypes.string, C, embedding_size=2, vocab=V[:5])]
    return TwoTowerModel(qf, cf, "art", 6, [12], [12], device=CPU, seed=0, **kw)


def test_region_plan_of_a_model():
    m = _model()
    descs = [clip_tower_desc(m.query_tower, "query", 16), clip_tower_desc(m.candidate_tower, "candidate", 16 + 4)]
    names, regions = plan_clip_regions(descs)
    dq, dc = m.query_tower.input_layer.output_dim, m.candidate_tower.input_layer.output_dim
    # the doubled name keeps the last declaration's table (dim 2), looked up twice
    assert (dq, dc) == (1 + 8 + 4, 8 + 2 + 2)
    assert names == ["query/dense_0/kernel", "query/dense_0/bias", "query/dense_1/kernel", "query/dense_1/bias",
                     "query/embedding/cust", "query/embedding/hist",
                     "candidate/dense_0/kernel", "candidate/dense_0/bias", "candidate/dense_1/kernel",
                     "candidate/dense_1/bias", "candidate/embedding/art", "candidate/embedding/ptn"]
    dense = [r for r in regions if r["kind"] == "dense"]
    assert [(r["tower"], r["var"], r["start"], r["size"]) for r in dense] == [
        (0, 0, 0, dq * 12), (0, 1, dq * 12, 12), (0, 2, dq * 12 + 12, 12 * 6), (0, 3, dq * 12 + 12 + 72, 6),
        (1, 6, 0, dc * 12), (1, 7, dc * 12, 12), (1, 8, dc * 12 + 12, 12 * 6), (1, 9, dc * 12 + 12 + 72, 6)]
    for t in (m.query_tower, m.candidate_tower):  # the dense regions tile flat exactly
        ti = 0 if t is m.query_tower else 1
        spans = sorted((r["start"], r["start"] + r["size"]) for r in dense if r["tower"] == ti)
        assert spans[0][0] == 0 and spans[-1][1] == t.dense.flat.numel()
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    rest = [r for r in regions if r["kind"] != "dense"]
    assert rest == [
        dict(var=4, tower=0, kind="input", col=1, cols=8, rows=16),    # cust, after the numeric column
        dict(var=5, tower=0, kind="bag", bag=0, cols=4, rows=16 * 5),  # hist: the expanded rows
        dict(var=10, tower=1, kind="input", col=0, cols=8, rows=20),
        dict(var=11, tower=1, kind="input", col=8, cols=2, rows=20),   # ptn twice: ONE variable
        dict(var=11, tower=1, kind="input", col=10, cols=2, rows=20)]
    # no region covers the numeric column 0 of the query tower's input gradient
    assert all(r["col"] >= 1 for r in rest if r["tower"] == 0 and r["kind"] == "input")
    assert not any(r["kind"] == "input" and r["tower"] == 0 and r["col"] <= 0 < r["col"] + r["cols"] for r in rest)


def test_region_plan_without_gradients():
    m = _model()
    names, regions = plan_clip_regions([clip_tower_desc(m.query_tower, "query", None, dense=False),
                                        clip_tower_desc(m.candidate_tower, "candidate", 8)])
    assert names[:2] == ["query/embedding/cust", "query/embedding/hist"]  # named, with no region
    assert all(r["tower"] == 1 for r in regions) and len(regions) == 4 + 3


def test_fused_optimizer_apply_is_refused():
    m = _model(fused_optimizer_apply=True)
    with pytest.raises(ValueError, match="fused_optimizer_apply"):
        m.compile(optimizer=Adagrad(learning_rate=0.1, clipnorm=1.0))
    m.compile(optimizer=Adagrad(learning_rate=0.1))  # without clipping: as before
    m.optimizer = Adagrad(learning_rate=0.1, global_clipnorm=1.0)  # set behind compile's back
    with pytest.raises(ValueError, match="fused_optimizer_apply"):
        m.train_step({})


def test_sharded_step_is_refused():
    from pkg.modelling.distributed import ShardedTrainStep

    qf = [Feature("cust", dtypes.string, Q, embedding_size=8, vocab=V)]
    cf = [Feature("art", dtypes.string, C, embedding_size=8, vocab=V)]
    m = TwoTowerModel(qf, cf, "art", 6, [12], [12], device=CPU, seed=0)
    m.compile(optimizer=Adagrad(learning_rate=0.1, clipvalue=1.0))
    with pytest.raises(NotImplementedError, match="gradient clipping"):
        ShardedTrainStep(m)


def test_restatement_against_a_naive_loop():
    rng = np.random.default_rng(0)
    vs = [[(rng.standard_normal(37) * 10).astype(np.float32), rng.standard_normal((5, 3)).astype(np.float32)],
          [np.zeros(4, np.float32)], [np.array([3.0, 4.0], np.float32)]]
    for cv in (None, 0.75):
        for v in vs:
            a, b = ref.sumsq(v, cv), ref.naive_sumsq(v, cv)
            assert abs(a - b) <= 64 * 2.0 ** -53 * a
    ss, fs, out = ref.clip(vs, clipvalue=None, clipnorm=5.0)
    assert ss[2] == 25.0 and fs[2] == np.float32(1.0) and fs[1] == np.float32(1.0)  # n == c; all zero
    assert fs[0] == np.float32(5.0) / np.float32(math.sqrt(ss[0])) and fs[0] < 1
    assert np.array_equal(out[0][1], vs[0][1] * fs[0])
    ss, fs, out = ref.clip(vs, clipvalue=1.0, global_clipnorm=2.0)
    total = sum(ref.naive_sumsq(v, 1.0) for v in vs)
    assert len(set(fs)) == 1 and abs(float(fs[0]) - 2.0 / math.sqrt(total)) < 1e-6
    assert np.array_equal(out[2][0], np.array([1.0, 1.0], np.float32) * fs[0])
    assert ref.factor(0.0, 1.0) == np.float32(1.0)
    assert ref.factor(2.0, 1.0).tobytes() in ref.factor_candidates(2.0, 1.0)


def test_region_struct_and_exports():
    assert ctypes.sizeof(_native.ClipRegion) == 48 and _native.MAX_CLIP_REGIONS == 32
    for name in ("tt_grad_sumsq", "tt_grad_clip_apply", "tt_grad_clip_workspace_size"):
        assert name in _native.EXPORTED_SYMBOLS


def test_entry_argument_checks():
    lib = _native.lib()
    one = ctypes.c_void_p(256)  # never dereferenced: every call below fails its host checks
    r = (_native.ClipRegion * 2)()
    r[0].g, r[0].rows, r[0].cols, r[0].ld, r[0].var = 256, 4, 8, 8, 0
    r[1].g, r[1].rows, r[1].cols, r[1].ld, r[1].var = 256, 1, 5000, 5000, 1
    # 8 chunks -> 1 workgroup; 1250 chunks -> 2: one fp64 partial each
    assert lib.tt_grad_clip_workspace_size(r, 2) == 256
    big = (_native.ClipRegion * 1)()
    big[0].g, big[0].rows, big[0].cols, big[0].ld = 256, 1, 1 << 30, 1 << 30
    assert lib.tt_grad_clip_workspace_size(big, 1) == 256 * 8  # the per-region grid cap

    def bad(rc, word):
        assert rc == _native.TT_ERR_BAD_ARG
        assert word in lib.tt_last_error().decode(), lib.tt_last_error().decode()

    bad(lib.tt_grad_sumsq(None, 2, 2, 0.0, one, one, 1 << 20, None), "NULL regions")
    bad(lib.tt_grad_sumsq(r, 2, 2, 0.0, None, one, 1 << 20, None), "NULL sumsq")
    bad(lib.tt_grad_sumsq(r, 2, 2, 0.0, one, None, 1 << 20, None), "NULL workspace")
    bad(lib.tt_grad_sumsq(r, 2, 1, 0.0, one, one, 1 << 20, None), "var=1 outside")
    bad(lib.tt_grad_sumsq(r, -1, 2, 0.0, one, one, 1 << 20, None), "negative")
    bad(lib.tt_grad_sumsq(r, 2, 0, 0.0, one, one, 1 << 20, None), "num_vars")
    assert lib.tt_grad_sumsq(r, 2, 2, 0.0, one, one, 8, None) == _native.TT_ERR_WORKSPACE
    r[0].rows = -1
    bad(lib.tt_grad_sumsq(r, 2, 2, 0.0, one, one, 1 << 20, None), "negative size")
    bad(lib.tt_grad_clip_apply(r, 2, 2, 0.0, 1.0, 0.0, one, one, None), "negative size")
    r[0].rows, r[0].ld = 4, 7
    bad(lib.tt_grad_clip_apply(r, 2, 2, 0.0, 1.0, 0.0, one, one, None), "ld=7 below cols=8")
    r[0].ld, r[0].g = 8, None
    bad(lib.tt_grad_clip_apply(r, 2, 2, 0.0, 1.0, 0.0, one, one, None), "g is NULL")
    r[0].g = 256
    bad(lib.tt_grad_clip_apply(r, 2, 2, 0.0, 1.0, 0.0, None, one, None), "sumsq is NULL")
    bad(lib.tt_grad_clip_apply(r, 2, 2, 0.0, 1.0, 1.0, one, one, None), "both")
    bad(lib.tt_grad_clip_apply(r, 2, 2, float("nan"), 0.0, 0.0, None, one, None), "NaN")
    r[1].var = 2
    bad(lib.tt_grad_clip_apply(r, 2, 2, 1.0, 0.0, 0.0, None, None, None), "var=2 outside")
    big[0].rows, big[0].cols, big[0].ld = 1 << 31, 8, 8
    assert lib.tt_grad_sumsq(big, 1, 1, 0.0, one, one, 1 << 20, None) == _native.TT_ERR_UNSUPPORTED
