"""CPU: per-example sample weights on the host side: the fold's algebra against
fp64 autograd, encode_dataframe's checks and normalisation, the dataset's
recorded scale through save / load / map, the C entry's argument checks (no
kernel is launched by them) and the rank-sharded loss over gloo with the CPU
restatements injected."""
import ctypes
import os
import socket

import numpy as np
import pandas as pd
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import weight_ref
from pkg import _native, dtypes
from pkg.modelling.dataset import EncodedDataset, encode_dataframe
from pkg.schema.features import Feature, FeatureFamily


def _problem(B, E, seed=0, zeros=True):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((B, E))
    c = rng.standard_normal((B, E))
    logq = np.log(rng.dirichlet(np.ones(B)))
    w = rng.uniform(0.0, 3.0, B)
    if zeros:
        w[rng.choice(B, max(B // 8, 1), replace=False)] = 0.0
    return q, c, logq, w


def test_fold_into_cols_formula_reproduces_autograd_dc():
    """The fp32 fold of fp32 lse / row_loss, handed to the fp64 cols formula,
    is the weighted loss's dC (times w_max) and w * dq its dQ."""
    B, E = 96, 32
    q, c, logq, w = _problem(B, E)
    assert (w == 0).any() and w.max() > 1
    ref = weight_ref.weighted_ref(q, c, logq, w)
    plain = weight_ref.weighted_ref(q, c, logq)
    w_max = np.float32(w.max())
    wn = w.astype(np.float32) / w_max
    lse_w, row_loss_w, wloss = weight_ref.fold(wn, plain["lse"].astype(np.float32),
                                               plain["row_loss"].astype(np.float32))
    dc = float(w_max) * weight_ref.cols_formula(q, lse_w, row_loss_w, c, logq)
    err = np.abs(dc - ref["dc"]).max() / np.abs(ref["dc"]).max()
    print(f"fold -> cols formula: dC relative error {err:.3g}")
    assert err <= 1e-5  # 1.5e-6 measured: fp32 lse alone
    dq = float(w_max) * weight_ref.scale_rows(wn.astype(np.float64), plain["dq"])
    assert np.abs(dq - ref["dq"]).max() <= 1e-6 * np.abs(ref["dq"]).max()
    assert abs(float(w_max) * wloss.astype(np.float64).sum() - ref["loss"]) <= 1e-6 * abs(ref["loss"])
    # weight-0 rows contribute exactly nothing: another q in those rows, the same dC
    z = w == 0
    q2 = q.copy()
    q2[z] = 7.0 * np.random.default_rng(5).standard_normal((int(z.sum()), E))
    assert np.array_equal(weight_ref.cols_formula(q2, lse_w, row_loss_w, c, logq),
                          weight_ref.cols_formula(q, lse_w, row_loss_w, c, logq))


def test_fold_contract_rows():
    w = np.array([1.0, 0.0, 0.25, -1.0, 1.5, np.nan, -0.0], np.float32)
    lse = np.linspace(-3, 9, 7).astype(np.float32)
    rl = np.array([100.0, 3.0, 0.5, 1.0, 1.0, 1.0, 2.0], np.float32)
    lw, rw, wl = weight_ref.fold(w, lse, rl)
    assert (lw[0], rw[0], wl[0]) == (lse[0], rl[0], rl[0])  # the copy: log1p(expm1(-100)) would be -inf
    for i in (1, 6):
        assert lw[i] == np.inf and rw[i] == 0 and wl[i] == 0 and not np.signbit(rw[i]) and not np.signbit(wl[i])
    assert wl[2] == np.float32(0.25) * rl[2] and lw[2] == lse[2] - np.log(np.float32(0.25))
    assert np.isclose(-np.expm1(-np.float64(rw[2])), 0.25 * -np.expm1(-0.5), rtol=1e-6)
    assert np.isnan(lw[3:6]).all() and np.isnan(rw[3:6]).all() and np.isnan(wl[3:6]).all()
    dq = np.arange(14, dtype=np.float32).reshape(7, 2)
    dq[1] = np.nan
    out = weight_ref.scale_rows(w, dq)
    assert np.array_equal(out[0], dq[0]) and np.array_equal(out[1], [0, 0]) and np.array_equal(out[2], dq[2] * w[2])
    assert np.isnan(out[3:6]).all() and np.array_equal(out[6], [0, 0])


# ---- encode_dataframe / datasets ------------------------------------------------------------
FEATS = [Feature("x", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=["a", "b", "c"])]


def _frame(w):
    return pd.DataFrame({"x": ["a", "b", "c", "zz"][:len(w)], "recency": w})


def test_encode_dataframe_normalises_and_records_the_scale():
    w = [0.5, 3.0, 0.0, 1.5]
    cols = encode_dataframe(_frame(w), FEATS, sample_weight="recency")
    assert cols["__weight__"].dtype == np.float32
    assert np.array_equal(cols["__weight__"], np.asarray(w, np.float32) / np.float32(3.0))
    assert cols.weight_scale == 3.0 and cols["__weight__"].max() == 1.0
    assert cols["x"].tolist() == [1, 2, 3, 0]
    by_array = encode_dataframe(_frame(w), FEATS, sample_weight=np.asarray(w, np.float64))
    assert np.array_equal(by_array["__weight__"], cols["__weight__"]) and by_array.weight_scale == 3.0
    # a scale that fp32 does not hold exactly: the recorded scale is the fp32 divisor
    cols = encode_dataframe(_frame([0.1, 0.3, 0.2, 0.3]), FEATS, sample_weight="recency")
    assert cols.weight_scale == float(np.float32(0.3))
    assert np.array_equal(cols["__weight__"], np.asarray([0.1, 0.3, 0.2, 0.3], np.float32) / np.float32(0.3))
    plain = encode_dataframe(_frame(w), FEATS)
    assert "__weight__" not in plain and plain.weight_scale is None
    assert EncodedDataset(plain).weight_scale is None


@pytest.mark.parametrize("w,row", [([1.0, -0.5, 2.0, -1.0], 1), ([1.0, 2.0, float("nan"), 1.0], 2),
                                   ([1.0, 2.0, 3.0, float("inf")], 3), ([0.0, 0.0, 0.0, 0.0], 0)])
def test_encode_dataframe_refuses_bad_weights(w, row):
    with pytest.raises(ValueError, match=f"row {row} "):
        encode_dataframe(_frame(w), FEATS, sample_weight="recency")


def test_encode_dataframe_refuses_a_wrong_length():
    with pytest.raises(ValueError, match="rows"):
        encode_dataframe(_frame([1.0, 2.0, 3.0, 4.0]), FEATS, sample_weight=np.ones(3))


def test_scale_survives_save_load_and_map(tmp_path):
    cols = encode_dataframe(_frame([0.5, 2.5, 0.0, 1.0]), FEATS, sample_weight="recency")
    ds = EncodedDataset(cols, batch_size=2, device=torch.device("cpu"))
    assert ds.weight_scale == 2.5
    assert ds.map(lambda b: b).weight_scale == 2.5
    ds.save(str(tmp_path / "w"), max_rows=3)  # two shards, each carrying the scale
    back = EncodedDataset.load(str(tmp_path / "w"), batch_size=2, device=torch.device("cpu"))
    assert back.weight_scale == 2.5 and back.num_rows == 4
    assert sorted(back.columns) == ["__weight__", "x"]  # the scale is no column
    assert np.array_equal(back.columns["__weight__"], cols["__weight__"])
    batches = list(back)
    assert torch.equal(batches[1]["__weight__"], torch.tensor([0.0, 0.4]))
    # unweighted datasets are stored as before
    plain = EncodedDataset(encode_dataframe(_frame([1.0] * 4), FEATS), device=torch.device("cpu"))
    plain.save(str(tmp_path / "p"))
    assert EncodedDataset.load(str(tmp_path / "p"), device=torch.device("cpu")).weight_scale is None
    with np.load(str(tmp_path / "p" / "part-00000.npz")) as z:
        assert sorted(z.files) == ["x"]


# ---- the C entry's argument checks ------------------------------------------------------------
def test_c_entry_refuses_bad_arguments():
    lib = _native.lib()
    fn = lib.tt_inbatch_weight_rows
    bad = _native.TT_ERR_BAD_ARG
    p = 4096  # never dereferenced: every call below returns before a launch
    assert fn(None, p, p, 4, p, p, p, None, 0, 0, None) == bad and "NULL" in lib.tt_last_error().decode()
    assert fn(p, None, p, 4, p, p, p, None, 0, 0, None) == bad
    assert fn(p, p, None, 4, p, p, p, None, 0, 0, None) == bad
    assert fn(None, None, None, 4, None, None, None, None, 0, 0, None) == bad
    assert fn(p, p, p, -1, p, p, p, None, 0, 0, None) == bad and "n=-1" in lib.tt_last_error().decode()
    assert fn(p, p, p, 4, p, p, p, p, 8, -1, None) == bad and "dim=-1" in lib.tt_last_error().decode()
    assert fn(p, p, p, 4, p, p, p, p, 7, 8, None) == bad and "lddq=7" in lib.tt_last_error().decode()
    assert fn(p, p, p, 0, p, p, None, None, 0, 0, None) == _native.TT_OK  # n == 0: no work
    assert fn(p, p, p, 0, p, p, p, p, 8, 8, None) == _native.TT_OK
    assert fn(None, None, None, 0, None, None, None, None, 0, 0, None) == _native.TT_OK  # pointers not looked at
    assert fn(None, None, None, 0, None, None, None, None, 7, 8, None) == bad  # the shape checks come first
    with pytest.raises(_native.TTError):
        _native.check(fn(p, p, p, -1, p, p, p, None, 0, 0, None))
    assert "tt_inbatch_weight_rows" in _native.EXPORTED_SYMBOLS
    assert isinstance(fn, ctypes._CFuncPtr)


# ---- the rank-sharded loss over gloo ------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _global_loss_worker(rank, world, port, q, c, logq, w, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from oracle import oracle
    from pkg.modelling.distributed import BatchComm
    from pkg.modelling.losses import global_inbatch_grads

    def rows(qq, C, L, pos_offset):  # as tests/test_distributed_gloo.py builds it
        r = oracle.inbatch_softmax_xent(qq.numpy(), C.numpy(), None if L is None else L.numpy(), pos_offset)
        return torch.from_numpy(r["lse"]), torch.from_numpy(r["row_loss"]), torch.from_numpy(r["dq"])

    def cols(Qa, lse, cl, L, pos_offset, row_loss=None):  # reads row_loss where the kernel does
        return torch.from_numpy(weight_ref.cols_formula(Qa.numpy(), lse.numpy(), row_loss.numpy(), cl.numpy(),
                                                        None if L is None else L.numpy(), pos_offset))

    def fold(ww, lse, row_loss, dq):
        lw, rw, wl = weight_ref.fold(ww.numpy(), lse.numpy(), row_loss.numpy(), np.float64)
        dq.copy_(torch.from_numpy(weight_ref.scale_rows(ww.numpy(), dq.numpy())))  # in place, as the kernel
        return torch.from_numpy(lw), torch.from_numpy(rw), torch.from_numpy(wl)

    b = q.shape[0] // world
    sl = slice(rank * b, (rank + 1) * b)
    wloss, dq, dc = global_inbatch_grads(torch.from_numpy(q[sl]), torch.from_numpy(c[sl]), torch.from_numpy(logq[sl]),
                                         BatchComm(), rows, cols, weights=torch.from_numpy(w[sl]), fold=fold)
    out[rank] = (wloss.numpy(), dq.numpy(), dc.numpy())
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_global_negatives_weighted_loss_equals_full_batch(world):
    """global_inbatch_grads(weights=...) over gloo, CPU rows / fold / cols
    injected: every rank's weighted loss terms, dq and dc equal the
    single-process fp64 autograd result of the whole batch."""
    rng = np.random.default_rng(2)
    B, E = 12 * world, 8
    q = rng.standard_normal((B, E))
    c = rng.standard_normal((B, E))
    logq = np.log(rng.dirichlet(np.ones(B)))
    w = rng.uniform(0.0, 1.0, B)
    w[[1, B // 2, B - 1]] = 0.0
    w[[0, B // 2 + 1]] = 1.0
    ref = weight_ref.weighted_ref(q, c, logq, w)
    out = mp.Manager().dict()
    mp.spawn(_global_loss_worker, args=(world, _free_port(), q, c, logq, w, out), nprocs=world, join=True)
    b = B // world
    total = 0.0
    for r in range(world):
        wl, dq, dc = out[r]
        sl = slice(r * b, (r + 1) * b)
        np.testing.assert_allclose(wl, (w * ref["row_loss"])[sl], rtol=1e-12)
        np.testing.assert_allclose(dq, ref["dq"][sl], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(dc, ref["dc"][sl], rtol=1e-10, atol=1e-12)
        total += wl.sum()
    assert abs(total - ref["loss"]) <= 1e-10 * abs(ref["loss"])


def test_sharded_train_step_refuses_weighted_batches():
    """The check comes before the step looks at any of its state (or at a
    process group), so it is made on a bare instance."""
    from pkg.modelling.distributed import ShardedTrainStep

    step = ShardedTrainStep.__new__(ShardedTrainStep)
    with pytest.raises(NotImplementedError, match="__weight__"):
        step({"cust": None, "__weight__": None})
