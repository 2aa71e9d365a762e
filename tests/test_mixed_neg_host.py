"""Mixed negative sampling (TwoTowerModel(num_sampled_negatives=M)) on the
host: the sampler's restatement (tests/mixed_neg_ref.py) against the published
Philox4x32-10 known answers and its uniformity, the mixture's logQ table, the
candidate catalogue, every argument check and the native entries' host
validation.  No GPU."""
import ctypes
import logging

import numpy as np
import pandas as pd
import pytest
import torch

import mixed_neg_ref as mn
from pkg import _native, dtypes
from pkg.modelling.dataset import CandidateCatalogue, encode_dataframe
from pkg.modelling.models.two_tower_model import LOGQ_KEY, TwoTowerModel
from pkg.modelling.optimizer_factory import OptimizerFactory
from pkg.schema.features import Feature, FeatureFamily


# --------------------------------------------------------------------------- the sampler
def test_philox_known_answers():
    zero = mn.philox4x32_10([0, 0, 0, 0], [0, 0])
    assert [f"{int(w):08x}" for w in zero] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = mn.philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)
    assert [f"{int(w):08x}" for w in ones] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]


def test_sampler_counter_layout():
    """Slot m is word m & 3 of block m >> 2; the step fills counter words 1, 2
    and the seed the key, low word first."""
    seed, step = 0x1234567800000009, 0x0000000500000007
    u = mn.words(11, seed, step)
    for m in (0, 1, 5, 10):
        blk = mn.philox4x32_10([m >> 2, 7, 5, 0], [9, 0x12345678])
        assert int(u[m]) == int(blk[m & 3])
    s = mn.sample(11, 1000, seed, step)
    assert [int(x) for x in s] == [(int(w) * 1000) >> 32 for w in u]


@pytest.mark.parametrize("seed,step", [(0, 0), (0, 1), (1234, 7)])
def test_sampler_is_uniform(seed, step):
    """N = 1000, 2^20 draws: every bin within 5 sigma of its mean and
    chi^2 <= 999 + 5 sqrt(1998)."""
    N, draws = 1000, 1 << 20
    counts = np.bincount(mn.sample(draws, N, seed, step), minlength=N)
    assert counts.shape == (N,) and counts.sum() == draws
    mean = draws / N
    sigma = np.sqrt(draws * (1 / N) * (1 - 1 / N))
    dev = np.abs(counts - mean).max() / sigma
    chi2 = float(((counts - mean) ** 2 / mean).sum())
    print(f"seed {seed} step {step}: max deviation {dev:.2f} sigma, chi^2 {chi2:.1f}")
    assert dev <= 5.0
    assert chi2 <= 999 + 5 * np.sqrt(1998)


def test_consecutive_steps_share_no_slot():
    a, b = mn.sample(4096, 105542, 0, 0), mn.sample(4096, 105542, 0, 1)
    assert int((a == b).sum()) == 0
    assert a.min() >= 0 and a.max() < 105542


def test_sample_edges():
    assert (mn.sample(64, 1, 3, 4) == 0).all()
    s = mn.sample(4096, (1 << 31) - 1, 0, 0)
    assert s.min() >= 0 and s.max() < (1 << 31) - 1


# --------------------------------------------------------------------------- the model's interface
V = [str(i) for i in range(300)]


def _features(seq=False):
    qf = [Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V)]
    cf = [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=V),
          Feature("price", dtypes.float32, FeatureFamily.CANDIDATE),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=4, vocab=V[:20])]
    if seq:
        cf.append(Feature("hist", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=4, vocab=V[:20],
                          sequence_length=3))
    return qf, cf


def _model(probs=None, seq=False, **kw):
    qf, cf = _features(seq)
    m = TwoTowerModel(qf, cf, "art", 8, [8], [8], probs, device=torch.device("cpu"), seed=0, **kw)
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", {"learning_rate": 0.05}))
    return m


def _frame(n=50, seed=0):
    rng = np.random.default_rng(seed)
    return pd.DataFrame({"art": [str(i) for i in rng.integers(0, 320, n)],  # some outside the vocab
                         "price": rng.uniform(0, 1, n).astype(np.float32),
                         "ptn": [str(i) for i in rng.integers(0, 25, n)]})


@pytest.mark.parametrize("m", [0, -1, 2.5, True, "4"])
def test_model_refuses_a_bad_m(m):
    with pytest.raises(ValueError, match="num_sampled_negatives"):
        _model(num_sampled_negatives=m)


def test_model_refuses_a_bad_seed():
    with pytest.raises(ValueError, match="sampled_negatives_seed"):
        _model(num_sampled_negatives=4, sampled_negatives_seed=1.5)


def test_model_defaults():
    m = _model()
    assert m.num_sampled_negatives is None and m.sampled_negatives_seed == 0 and m.candidate_catalogue is None
    m = _model(num_sampled_negatives=np.int64(40), sampled_negatives_seed=9)
    assert m.num_sampled_negatives == 40 and isinstance(m.num_sampled_negatives, int)
    assert m.sampled_negatives_seed == 9


def test_catalogue_from_dataframe_equals_encode_dataframe():
    _, cf = _features()
    df = _frame()
    cat = CandidateCatalogue.from_dataframe(df, cf, device=torch.device("cpu"))
    enc = encode_dataframe(df, cf)
    assert cat.feature_names == ["art", "price", "ptn"] and cat.num_rows == len(df) == len(cat)
    assert cat.words.dtype == torch.int32 and tuple(cat.words.shape) == (3, len(df))
    assert np.array_equal(cat.words[0].numpy(), enc["art"].astype(np.int32))
    assert np.array_equal(cat.words[1].numpy(), enc["price"].astype(np.float32).view(np.int32))
    assert np.array_equal(cat.words[2].numpy(), enc["ptn"].astype(np.int32))
    assert np.array_equal(cat.column("price").numpy(), enc["price"].astype(np.float32))
    # plain construction takes the encoded columns
    again = CandidateCatalogue(enc, cf, device=torch.device("cpu"))
    assert torch.equal(again.words, cat.words)


def test_catalogue_argument_checks():
    _, cf = _features()
    enc = encode_dataframe(_frame(), cf)
    with pytest.raises(ValueError, match="lacks"):
        CandidateCatalogue({k: v for k, v in enc.items() if k != "ptn"}, cf, device=torch.device("cpu"))
    with pytest.raises(TypeError, match="encoded"):
        CandidateCatalogue(dict(enc, art=np.asarray(["1"] * 50)), cf, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="outside"):
        CandidateCatalogue(dict(enc, ptn=np.full(50, 21)), cf, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="one length"):
        CandidateCatalogue(dict(enc, ptn=enc["ptn"][:10]), cf, device=torch.device("cpu"))


def test_sequence_feature_is_refused_by_name():
    _, cf = _features(seq=True)
    df = _frame()
    df["hist"] = [["1", "2"]] * len(df)
    with pytest.raises(NotImplementedError, match="hist"):
        CandidateCatalogue.from_dataframe(df, cf, device=torch.device("cpu"))
    m = _model(seq=True, num_sampled_negatives=4)
    cat = CandidateCatalogue.from_dataframe(_frame(), _features()[1], device=torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="hist"):
        m.set_candidate_catalogue(cat)


def test_set_candidate_catalogue_checks():
    m = _model(num_sampled_negatives=4)
    with pytest.raises(TypeError):
        m.set_candidate_catalogue({"art": np.zeros(3)})
    _, cf = _features()
    with pytest.raises(ValueError, match="candidate tower takes"):
        m.set_candidate_catalogue(CandidateCatalogue.from_dataframe(_frame(), cf[:2], device=torch.device("cpu")))
    cat = CandidateCatalogue.from_dataframe(_frame(), cf, device=torch.device("cpu"))
    m.set_candidate_catalogue(cat)
    assert m.candidate_catalogue is cat and int(m._mixed_step.item()) == 0


def _batch(n=16):
    rng = np.random.default_rng(1)
    return {"cust": rng.integers(0, 301, n).astype(np.int32), "art": rng.integers(0, 301, n).astype(np.int32),
            "price": rng.uniform(0, 1, n).astype(np.float32), "ptn": rng.integers(0, 21, n).astype(np.int32)}


def test_training_without_a_catalogue_raises():
    m = _model(num_sampled_negatives=4)
    with pytest.raises(RuntimeError, match="set_candidate_catalogue"):
        m.train_step(_batch())


def test_batch_with_logq_column_is_refused():
    probs = {v: 1.0 / 300 for v in V}
    m = _model(probs, num_sampled_negatives=4)
    m.set_candidate_catalogue(CandidateCatalogue.from_dataframe(_frame(), _features()[1], device=torch.device("cpu")))
    x = _batch()
    x[LOGQ_KEY] = np.zeros(16, np.float32)
    with pytest.raises(ValueError, match="__logq__"):
        m.train_step(x)


def test_one_warning_without_hit_removal(caplog):
    with caplog.at_level(logging.WARNING, logger="pkg.modelling.models.two_tower_model"):
        m = _model(num_sampled_negatives=4)
        m.compile()
        m.compile()
    assert sum("remove_accidental_hits" in r.getMessage() for r in caplog.records) == 1
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="pkg.modelling.models.two_tower_model"):
        _model(num_sampled_negatives=4, remove_accidental_hits=True)
        _model()
    assert not [r for r in caplog.records if "remove_accidental_hits" in r.getMessage()]


def test_mixture_logq_table_against_fp64():
    rng = np.random.default_rng(5)
    known = V[:250]  # the other 50 vocab entries are outside the lookup: p = 1
    probs = {v: float(p) for v, p in zip(known, rng.dirichlet(np.ones(250)))}
    m = _model(probs, num_sampled_negatives=40)
    cat = CandidateCatalogue.from_dataframe(_frame(77), _features()[1], device=torch.device("cpu"))
    m.set_candidate_catalogue(cat)
    p = np.ones(301)
    p[1:251] = np.asarray([probs[v] for v in known], np.float32).astype(np.float64)
    for B in (96, 33):  # the eager partial last batch has another B
        t = m.mixture_logq_table(B)
        want = mn.mixture_logq(p, B, 40, 77)
        assert t.dtype == torch.float32 and tuple(t.shape) == (301,)
        assert np.array_equal(t.numpy(), want.astype(np.float32))
        assert m.mixture_logq_table(B) is t  # cached per (B, M)
    assert m.mixture_logq_table(96) is not m.mixture_logq_table(33)
    # rows outside the lookup (and the OOV row): p = 1
    assert float(m.mixture_logq_table(96)[0]) == np.float32(np.log((96 + 40 / 77) / 136))
    assert float(m.mixture_logq_table(96)[300]) == float(m.mixture_logq_table(96)[0])
    # plain in-batch sampling is the M -> 0 limit: log p
    assert np.allclose(mn.mixture_logq(p, 96, 0, 77), np.log(p))


def test_save_load_keeps_m_and_seed(tmp_path):
    m = _model(num_sampled_negatives=40, sampled_negatives_seed=1234)
    m.set_candidate_catalogue(CandidateCatalogue.from_dataframe(_frame(), _features()[1], device=torch.device("cpu")))
    m.save(str(tmp_path / "m"))
    r = TwoTowerModel.load(str(tmp_path / "m"), device=torch.device("cpu"))
    assert r.num_sampled_negatives == 40 and r.sampled_negatives_seed == 1234
    assert r.candidate_catalogue is None  # the catalogue is not saved
    d = _model()
    d.save(str(tmp_path / "d"))
    r = TwoTowerModel.load(str(tmp_path / "d"), device=torch.device("cpu"))
    assert r.num_sampled_negatives is None and r.sampled_negatives_seed == 0


# --------------------------------------------------------------------------- the sharded refusals
def test_global_inbatch_grads_refuses_extra_negatives():
    from pkg.modelling import losses

    class Comm:
        world, rank = 1, 0

    with pytest.raises(NotImplementedError, match="single-device"):
        losses.global_inbatch_grads(torch.zeros(4, 8), torch.zeros(6, 8), None, Comm())


def test_sharded_step_refuses_mixed_mode():
    from pkg.modelling.distributed import ShardedTrainStep

    with pytest.raises(NotImplementedError, match="mixed negative sampling"):
        ShardedTrainStep(_model(num_sampled_negatives=4))


# --------------------------------------------------------------------------- the native entries' host validation
def test_native_entries_validate_on_the_host():
    lib = _native.lib()
    one = ctypes.c_void_p(256)
    BAD, UNS = _native.TT_ERR_BAD_ARG, _native.TT_ERR_UNSUPPORTED
    # cols_mixed: NULL operands, ids that do not go together, dim > 128; the positives' range is NOT checked
    assert lib.tt_inbatch_xent_cols_mixed(None, 8, 4, one, None, one, 8, 6, 8, None, 0, None, None, 0, None, one,
                                          one, 1 << 30, None) == BAD
    assert lib.tt_inbatch_xent_cols_mixed(one, 8, 4, one, None, one, 8, 6, 8, None, 0, one, None, 0, None, one, one,
                                          1 << 30, None) == BAD
    assert "go together" in lib.tt_last_error().decode()
    assert lib.tt_inbatch_xent_cols_mixed(one, 256, 4, one, None, one, 256, 6, 256, None, 0, None, None, 0, None,
                                          one, one, 1 << 30, None) == UNS
    assert lib.tt_inbatch_xent_cols_mixed(one, 8, 4, one, None, one, 8, 6, 8, None, 0, None, None, 0, None, one,
                                          one, 16, None) == _native.TT_ERR_WORKSPACE  # n_cols > n_rows got this far
    assert lib.tt_inbatch_xent_cols(one, 8, 4, one, None, one, 8, 6, 8, None, 0, one, one, 1 << 30, None) == BAD
    # fused mixed
    def args(m, k, thr):
        return (one, 8, 4, one, 8, m, 8, None, None, 0, k, one, one, one, one, thr, 1.0, None, one, 16, None)

    assert lib.tt_inbatch_softmax_xent_mixed(*args(-1, 0, None)) == BAD
    assert lib.tt_inbatch_softmax_xent_mixed(*args(2, -1, None)) == BAD
    assert lib.tt_inbatch_softmax_xent_mixed(*args(2, 3, None)) == BAD
    assert "thr" in lib.tt_last_error().decode()
    assert lib.tt_inbatch_softmax_xent_mixed(*args(2, 0, None)) == _native.TT_ERR_WORKSPACE
    # workspaces: the mixed ones hold the hard ones' carve; m = 0 is the square fused entry's
    for x3 in (0, 1):
        assert lib.tt_inbatch_mixed_workspace_size(200, 448, 64, x3) == lib.tt_inbatch_hard_workspace_size(200, 448,
                                                                                                          64, x3)
        assert lib.tt_inbatch_fused_mixed_workspace_size(200, 0, 64, x3) == \
            lib.tt_inbatch_fused_hard_workspace_size(200, 64, x3)
        assert lib.tt_inbatch_fused_mixed_workspace_size(200, 300, 64, x3) > \
            lib.tt_inbatch_fused_mixed_workspace_size(200, 0, 64, x3)
    assert lib.tt_inbatch_fused_mixed_workspace_size(16, 4, 300, 0) == 0
    assert lib.tt_inbatch_fused_mixed_workspace_size(16, -1, 32, 0) == 0
    # the sampler
    ptrs = (ctypes.c_void_p * 2)(256, 512)
    ok = lambda **kw: lib.tt_mixed_candidates(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("cols", ptrs), ("cat", one), ("cat_ld", 100), ("ncols", 2), ("batch", 8), ("m", 4), ("n", 100), ("seed", 0),
        ("step", one), ("dst", one), ("dst_ld", 12), ("status", None), ("stream", None))])
    assert ok(ncols=0) == BAD and ok(ncols=33) == UNS
    assert ok(m=0) == BAD and ok(batch=0) == BAD
    assert ok(dst_ld=11) == BAD and ok(cat_ld=99) == BAD
    assert ok(step=None) == BAD and ok(cols=None) == BAD
    assert ok(n=0) == BAD and ok(n=1 << 31) == BAD  # without a status word to flag it in
    assert ok(cols=(ctypes.c_void_p * 2)(256, None)) == BAD
