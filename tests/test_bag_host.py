"""CPU: sequence features on the host side: Feature arguments, encoding,
vocabulary building, pickling and export specs, and the C entries' argument
checks (no kernel is launched by these calls)."""
import ctypes
import pickle

import numpy as np
import pandas as pd
import pytest

from pkg import _native, dtypes
from pkg.modelling import export
from pkg.schema.features import Feature, FeatureFamily

Q = FeatureFamily.QUERY
VOCAB = ["a", "b", "c", "d"]


def _hist(L=3, **kw):
    return Feature("hist", dtypes.string, Q, embedding_size=8, vocab=VOCAB, sequence_length=L, **kw)


def test_defaults_keep_existing_features():
    f = Feature("x", dtypes.string, Q, embedding_size=8, vocab=VOCAB)
    assert f.sequence_length is None and f.pooling == "mean" and not f.is_sequence
    assert f.encode(["a", "zz", "d"]).tolist() == [1, 0, 4]
    f = _hist(5, pooling="sqrtn")
    assert f.is_sequence and (f.sequence_length, f.pooling) == (5, "sqrtn")


def test_feature_argument_errors():
    with pytest.raises(ValueError, match="pooling"):
        _hist(pooling="max")
    with pytest.raises(ValueError, match="pooling"):
        Feature("x", dtypes.string, Q, embedding_size=8, vocab=VOCAB, pooling="max")
    with pytest.raises(TypeError, match="sequence_length"):
        _hist(L=2.0)
    with pytest.raises(TypeError, match="sequence_length"):
        _hist(L=True)
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError, match="sequence_length"):
            _hist(L=bad)
    with pytest.raises(TypeError, match="dtype must be tf.string"):
        Feature("age", dtypes.float32, Q, sequence_length=3)
    with pytest.raises(ValueError, match="embedding_size"):
        Feature("hist", dtypes.string, Q, vocab=VOCAB, sequence_length=3)
    assert _hist(L=1024).sequence_length == 1024


def test_encode_truncates_pads_and_maps_oov():
    f = _hist(3)
    out = f.encode([["a", "b", "c", "d"], ["b"], [], None, float("nan"), ("zz", "a"), np.array(["d", "d"])])
    assert out.dtype == np.int32 and out.shape == (7, 3)
    assert out.tolist() == [[2, 3, 4],      # the LAST three, in order
                            [2, -1, -1],    # left-aligned, padded with -1
                            [-1, -1, -1], [-1, -1, -1], [-1, -1, -1],
                            [0, 1, -1],     # unknown -> OOV row 0
                            [4, 4, -1]]
    assert f.encode([]).shape == (0, 3)
    assert f.encode(pd.Series([["a"], None])).tolist() == [[1, -1, -1], [-1, -1, -1]]
    # values are compared as str(), as everywhere
    g = Feature("hist", dtypes.string, Q, embedding_size=8, vocab=["7", "8"], sequence_length=2)
    assert g.encode([[7, 8, 9], [8]]).tolist() == [[2, 0], [2, -1]]
    assert g.encode(np.array([[7, 8], [9, 7]])).tolist() == [[1, 2], [0, 1]]
    with pytest.raises(TypeError, match="list, tuple or array"):
        f.encode(["a", "b"])


def test_encode_is_one_vocabulary_lookup(monkeypatch):
    f = _hist(3)
    f.encode([["a"]])
    calls = []
    real = f._native.encode
    monkeypatch.setattr(f._native, "encode", lambda v, n=0: calls.append(len(v)) or real(v, n))
    f.encode([["a", "b", "c", "d"], ["b"], []])
    assert calls == [4]  # the kept elements of every example, together


def test_set_vocab_from_dataframe_counts_elements():
    df = pd.DataFrame({"hist": [["x", "y"], ["x"], None, ["z", "x", "y"], []]})
    f = Feature("hist", dtypes.string, Q, embedding_size=8, sequence_length=2)
    f.set_vocab_from_dataframe(df)
    assert f.vocab.tolist() == ["x", "y", "z"] and f.is_built
    f = Feature("hist", dtypes.string, Q, embedding_size=8, sequence_length=2, max_vocab_size=2)
    f.set_vocab_from_dataframe(df)
    assert f.vocab.tolist() == ["x", "y"]
    assert f.encode(df["hist"]).tolist() == [[1, 2], [1, -1], [-1, -1], [1, 2], [-1, -1]]


def test_pickle_round_trip_and_old_pickles():
    f = pickle.loads(pickle.dumps(_hist(4, pooling="sum")))
    assert (f.sequence_length, f.pooling) == (4, "sum")
    assert f.encode([["a", "zz"]]).tolist() == [[1, 0, -1, -1]]
    old = Feature.__new__(Feature)
    state = _hist(4).__getstate__()
    del state["sequence_length"], state["pooling"]  # a pickle written before these fields
    old.__setstate__(state)
    assert old.sequence_length is None and old.pooling == "mean" and not old.is_sequence


def test_export_spec_round_trip_and_old_specs():
    f = _hist(4, pooling="sqrtn")
    spec = export._feature_spec(f)
    assert spec["sequence_length"] == 4 and spec["pooling"] == "sqrtn"
    arrays = export._vocab_arrays([f], "q.")
    (g,) = export._features_from([spec], arrays, "q.")
    assert (g.sequence_length, g.pooling, g.vocab.tolist()) == (4, "sqrtn", VOCAB)
    old = {k: v for k, v in spec.items() if k not in ("sequence_length", "pooling")}
    (h,) = export._features_from([old], arrays, "q.")
    assert h.sequence_length is None and h.pooling == "mean"
    plain = export._feature_spec(Feature("x", dtypes.string, Q, embedding_size=8, vocab=VOCAB))
    assert plain["sequence_length"] is None and plain["pooling"] == "mean"


def _job(**kw):
    j = (_native.BagJob * 1)()
    one = 1 << 12  # a non-NULL address; nothing is launched, so it is never read
    j[0].table, j[0].ids, j[0].out, j[0].scale_out = one, one, one, one
    j[0].num_rows, j[0].dim, j[0].L, j[0].out_stride, j[0].ids_row_stride, j[0].ids_pos_stride = 10, 8, 4, 8, 4, 1
    for k, v in kw.items():
        setattr(j[0], k, v)
    return j


def _grad_job(**kw):
    j = (_native.BagGradJob * 1)()
    one = 1 << 12
    j[0].ids, j[0].dout, j[0].scale, j[0].ids_flat, j[0].grad = one, one, one, one, one
    j[0].num_rows, j[0].dim, j[0].L, j[0].dout_stride, j[0].ids_row_stride, j[0].ids_pos_stride = 10, 8, 4, 8, 4, 1
    for k, v in kw.items():
        setattr(j[0], k, v)
    return j


@pytest.mark.parametrize("entry,make", [("tt_gather_bag", _job), ("tt_bag_grad_expand", _grad_job)])
def test_c_entries_refuse_bad_arguments(entry, make):
    lib = _native.lib()
    fn = getattr(lib, entry)
    bad, unsupported = _native.TT_ERR_BAD_ARG, _native.TT_ERR_UNSUPPORTED
    assert fn(None, 1, 4, None) == bad and "NULL jobs" in lib.tt_last_error().decode()
    assert fn(make(L=0), 1, 4, None) == bad and "L=0" in lib.tt_last_error().decode()
    assert fn(make(L=1025), 1, 4, None) == bad
    assert fn(make(L=1024), 1, 1 << 14, None) == bad and "2^24" in lib.tt_last_error().decode()  # batch * L = 2^24
    assert fn(make(L=4), 1, 1 << 22, None) == bad
    many = (type(make()[0]) * 9)()
    assert fn(many, 9, 4, None) == bad and "num_jobs" in lib.tt_last_error().decode()
    assert fn(make(), 0, 4, None) == bad
    assert fn(make(dim=0), 1, 4, None) == bad
    assert fn(make(dim=1025), 1, 4, None) == unsupported
    assert fn(make(pooling=3), 1, 4, None) == bad
    assert fn(make(num_rows=0), 1, 4, None) == bad
    assert fn(make(col_offset=1), 1, 4, None) == bad  # columns [1, 9) of an 8-wide row
    assert fn(make(ids=None), 1, 4, None) == bad
    assert fn(make(), 1, -1, None) == bad
    assert fn(make(), 1, 0, None) == _native.TT_OK  # batch 0: no work
    with pytest.raises(_native.TTError):
        _native.check(fn(make(L=0), 1, 4, None))


def test_gather_bag_refuses_a_null_table():
    lib = _native.lib()
    assert lib.tt_gather_bag(_job(table=None), 1, 4, None) == _native.TT_ERR_BAD_ARG
    assert "table is NULL" in lib.tt_last_error().decode()
    assert lib.tt_gather_bag(_job(table=None), 1, 0, None) == _native.TT_ERR_BAD_ARG  # even with no bags


def test_struct_layouts_match_the_header():
    # 8-byte pointers / int64, 4-byte int32: the field order of include/tt.h packs without holes
    assert ctypes.sizeof(_native.BagJob) == 80 and ctypes.sizeof(_native.BagGradJob) == 88
    assert _native.BAG_POOLINGS == {"sum": 0, "mean": 1, "sqrtn": 2} and _native.MAX_BAG_JOBS == 8


def test_sharded_step_refuses_a_sequence_feature():
    import torch

    from pkg.modelling.distributed import ShardedTrainStep
    from pkg.modelling.models.two_tower_model import TwoTowerModel
    from pkg.modelling.optimizer_factory import OptimizerFactory

    cf = [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=VOCAB)]
    with pytest.raises(ValueError, match="may not be a sequence feature"):
        TwoTowerModel([_hist(3)], [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8,
                                           vocab=VOCAB, sequence_length=2)], "art", 8, device=torch.device("cpu"))
    m = TwoTowerModel([_hist(3)], cf, "art", 8, device=torch.device("cpu"))
    assert m.get_input_signature()["hist"].shape == (None, 3) and m.get_input_signature()["art"].shape == (None, 1)
    assert [b for b in m.query_tower.input_layer.bag_sources()] == []
    assert m.query_tower.input_layer.output_dim == 8
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", {"learning_rate": 0.05}))
    with pytest.raises(NotImplementedError, match="'hist'"):
        ShardedTrainStep(m)
