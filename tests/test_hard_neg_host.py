"""CPU: hard-negative mining on the host side — the reference's own invariants
(tests/hard_neg_ref.py), the conditions the GPU cases rely on (exact inputs,
the certified gap of the end-to-end case), the rank-sharded loss over gloo
with CPU rows / cols / threshold injected, the keyword's validation and the C
entries' argument checks (no kernel is launched by them)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import hard_neg_ref as hn
import inbatch_rowwise
from pkg import _native

CPU = torch.device("cpu")


# ---- the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("hits", [False, True])
def test_select_invariants_on_exact_inputs(hits):
    n, E = 200, 32
    x = hn.to_torch(hn.exact_case(n, n, E, 0, hits), CPU)
    S = hn.scores(x["q"], x["c"], x["logq"], "fp64")
    # exact inputs: the three arithmetics give the same fp64 scores, each a float32 value
    assert torch.equal(S, hn.scores(x["q"], x["c"], x["logq"], "bf16"))
    assert torch.equal(S, hn.scores(x["q"], x["c"], x["logq"], "x3"))
    assert torch.equal(S, S.float().double())
    negs = n - 1
    hit = hn.hit_matrix(x["row_ids"], x["col_ids"], n, n, CPU)
    hit[torch.arange(n), torch.arange(n)] = False
    finite = negs - hit.sum(1)
    some_ties = False
    for k in (1, 2, 63, 64, 65, negs - 1, negs, negs + 5):
        sel = hn.select(S, k, 0, x["row_ids"], x["col_ids"])
        kept, thr = sel["kept"], sel["thr"]
        assert not bool(kept[torch.arange(n), torch.arange(n)].any())  # the positive is not a negative
        assert not bool((kept & hit).any())  # a hit is never kept
        none = torch.isinf(thr)
        # thr = -inf exactly where the (k+1)-th largest is -inf or missing: every finite negative kept
        assert bool((none == (finite <= k)).all())
        assert bool((kept.sum(1)[none] == finite[none]).all())
        # otherwise at least k kept, more only through ties at the k-th value
        cnt = kept.sum(1)[~none]
        assert bool((cnt >= k).all())
        a, b = sel["a"][~none], sel["b"][~none]
        assert bool(((cnt > k) == (a == b)).all())
        some_ties |= bool((cnt > k).any())
        assert bool((thr[~none].double() <= a).all()) and bool(((thr[~none].double() > b) | (a == b)).all())
    assert some_ties


def test_midpoint_that_rounds_to_b_becomes_a():
    b = np.float32(1.0)
    a = np.nextafter(b, np.float32(2.0))  # adjacent floats: the midpoint rounds to even = b
    S = torch.tensor([[9.0, float(a), float(b), 0.0]], dtype=torch.float64)  # column 0 the positive
    sel = hn.select(S, 1)
    assert float(sel["thr"][0]) == float(a)
    assert sel["kept"][0].tolist() == [False, True, False, False]
    sel = hn.select(S, 2)  # b = 1, next 0: thr = 0.5
    assert float(sel["thr"][0]) == 0.5 and sel["kept"][0].tolist() == [False, True, True, False]
    sel = hn.select(S, 3)  # as many negatives as k
    assert float(sel["thr"][0]) == float("-inf") and sel["kept"][0].tolist() == [False, True, True, True]


def test_reference_with_everything_kept_is_the_plain_reference():
    xc = inbatch_rowwise.case(129, 37, 0.45, True, True)
    q, c, logq = (torch.as_tensor(xc[k]) for k in ("q", "c", "logq"))
    ids = torch.as_tensor(xc["ids"])
    sel = hn.select(hn.scores(q, c, logq, "fp64"), 128, 0, ids, ids)
    assert bool(torch.isinf(sel["thr"]).all())
    got = hn.reference(q, c, logq, sel["kept"])
    want = inbatch_rowwise.reference_torch(q, c, logq, 0, ids, ids)
    for k in ("lse", "row_loss", "dq", "dc", "n"):
        assert torch.equal(got[k], want[k]), k


def test_masked_reference_matches_autograd():
    rng = np.random.default_rng(3)
    n, E, k = 40, 8, 5
    q, c = torch.as_tensor(rng.standard_normal((n, E))), torch.as_tensor(rng.standard_normal((n, E)))
    logq = torch.as_tensor(np.log(rng.dirichlet(np.ones(n))))
    sel = hn.select(hn.scores(q, c, logq, "fp64"), k)
    assert bool((sel["kept"].sum(1) == k).all())
    ref = hn.reference(q.float(), c.float(), logq.float(), sel["kept"])
    qa, ca = q.float().double().requires_grad_(), c.float().double().requires_grad_()
    S = qa @ ca.T - logq.float().double()[None, :]
    keep = sel["kept"] | torch.eye(n, dtype=torch.bool)
    loss = (torch.logsumexp(S.masked_fill(~keep, float("-inf")), 1) - S.diagonal()).sum()
    loss.backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-10 * abs(float(loss.detach()))
    np.testing.assert_allclose(ref["dq"].numpy(), qa.grad.numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(ref["dc"].numpy(), ca.grad.numpy(), rtol=1e-9, atol=1e-12)


# ---- what the GPU cases rely on ----------------------------------------------------------------------
@pytest.mark.parametrize("form", ["bf16", "x3"])
def test_gap_case_clears_64_delta_in_every_row(form):
    x = hn.to_torch(hn.gap_case(), CPU)
    sel = hn.select(hn.scores(x["q"], x["c"], x["logq"], "fp64"), hn.GAP_K)
    delta = hn.score_delta(x["q"], x["c"], form)
    gap = sel["a"] - sel["b"]
    print(f"{form}: min gap {float(gap.min()):.4g}, max 64 delta {float(64 * delta.max()):.4g}")
    assert bool((gap > 64 * delta).all())  # every row: none left out
    assert bool((sel["kept"].sum(1) == hn.GAP_K).all())
    ref = hn.reference(x["q"], x["c"], x["logq"], sel["kept"])
    assert bool(hn.bounds(ref, x["q"], x["c"], form)["certified"].all())


@pytest.mark.parametrize("E", [32, 64, 128])
def test_exact_cases_are_certified_in_both_forms(E):
    x = hn.to_torch(hn.exact_case(200, 200, E), CPU)
    S = hn.scores(x["q"], x["c"], x["logq"], "fp64")
    for k in (1, 64, 198):
        ref = hn.reference(x["q"], x["c"], x["logq"], hn.select(S, k)["kept"])
        for form in ("bf16", "x3"):
            assert bool(hn.bounds(ref, x["q"], x["c"], form)["certified"].all()), (E, k, form)


# ---- the rank-sharded loss over gloo -------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, c, logq, ids, k, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pkg.modelling.distributed import BatchComm
    from pkg.modelling.losses import global_inbatch_grads

    seen = {}

    def threshold(qq, C, L, kk, pos_offset, row_ids=None, col_ids=None):
        seen["k"] = kk
        return hn.select(hn.scores(qq, C, L, "fp64"), kk, pos_offset, row_ids, col_ids)["thr"]

    def _kept(qq, C, L, pos_offset, thr, row_ids, col_ids):
        S = hn.scores(qq, C, L, "fp64").masked_fill(hn.hit_matrix(row_ids, col_ids, qq.shape[0], C.shape[0], CPU),
                                                    float("-inf"))
        kept = (S >= thr.double()[:, None]) & torch.isfinite(S)
        kept[torch.arange(qq.shape[0]), torch.arange(qq.shape[0]) + pos_offset] = False
        return kept

    def rows(qq, C, L, pos_offset, thr, row_ids=None, col_ids=None):
        r = hn.reference(qq, C, L, _kept(qq, C, L, pos_offset, thr, row_ids, col_ids), pos_offset)
        return r["lse"], r["row_loss"], r["dq"]

    def cols(Qa, lse, cl, L, pos_offset, row_loss, thr, row_ids=None, col_ids=None):
        seen["thr_all"] = thr.clone()
        # the local columns against every row: S[i][j] for the rows' thr
        S = hn.scores(Qa, cl, L, "fp64")
        hit = hn.hit_matrix(row_ids, col_ids, Qa.shape[0], cl.shape[0], CPU)
        P = torch.exp(S - lse[:, None]).masked_fill(hit | (S < thr.double()[:, None]), 0.0)
        jj = torch.arange(cl.shape[0])
        P[jj + pos_offset, jj] = -(-torch.expm1(-row_loss[jj + pos_offset]))  # -(1 - P_pos)
        return P.T @ Qa.double()

    b = q.shape[0] // world
    sl = slice(rank * b, (rank + 1) * b)
    t = lambda a: None if a is None else torch.from_numpy(a[sl])  # noqa: E731
    row_loss, dq, dc = global_inbatch_grads(t(q), t(c), t(logq), BatchComm(), rows, cols, ids=t(ids),
                                            num_hard_negatives=k, threshold=threshold)
    out[rank] = (row_loss.numpy(), dq.numpy(), dc.numpy(), seen["thr_all"].numpy(), seen["k"])
    dist.destroy_process_group()


@pytest.mark.parametrize("hits", [False, True])
@pytest.mark.parametrize("world", [2, 3])
def test_global_negatives_hard_loss_equals_full_batch(world, hits):
    """global_inbatch_grads(num_hard_negatives=...) over gloo with CPU
    threshold / rows / cols injected: every rank's loss terms, dq and dc equal
    the single-process reference of the whole batch, and every rank's cols
    pass received every row's thr through the gather."""
    rng = np.random.default_rng(5 + world)
    B, E, k = 12 * world, 8, 4
    q = rng.standard_normal((B, E))
    c = rng.standard_normal((B, E))
    logq = np.log(rng.dirichlet(np.ones(B)))
    ids = rng.integers(0, B // 3, B).astype(np.int32) if hits else None
    tq, tc, tl = torch.from_numpy(q), torch.from_numpy(c), torch.from_numpy(logq)
    ti = None if ids is None else torch.from_numpy(ids)
    sel = hn.select(hn.scores(tq, tc, tl, "fp64"), k, 0, ti, ti)
    ref = inbatch_rowwise.to_numpy(hn.reference(tq, tc, tl, sel["kept"]))
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), q, c, logq, ids, k, out), nprocs=world, join=True)
    b = B // world
    for r in range(world):
        rl, dq, dc, thr_all, kk = out[r]
        sl = slice(r * b, (r + 1) * b)
        assert kk == k
        np.testing.assert_array_equal(thr_all.astype(np.float32), sel["thr"].numpy())
        np.testing.assert_allclose(rl, ref["row_loss"][sl], rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(dq, ref["dq"][sl], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(dc, ref["dc"][sl], rtol=1e-9, atol=1e-12)


# ---- validation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, -1, 2.5, True, "3"])
def test_losses_refuse_a_bad_k(k):
    from pkg.modelling import losses

    q = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="num_hard_negatives"):
        losses.inbatch_softmax_xent(q, q, None, num_hard_negatives=k)
    with pytest.raises(ValueError, match="num_hard_negatives"):
        losses.weighted_inbatch_grads(q, q, None, torch.ones(4), num_hard_negatives=k)
    with pytest.raises(ValueError, match="num_hard_negatives"):
        losses.global_inbatch_grads(q, q, None, None, num_hard_negatives=k)


@pytest.mark.parametrize("k", [0, -1, 2.5])
def test_model_refuses_a_bad_k(k):
    from pkg import dtypes
    from pkg.modelling.models.two_tower_model import TwoTowerModel
    from pkg.schema.features import Feature, FeatureFamily

    qf = Feature("u", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=["a", "b"])
    cf = Feature("i", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=["a", "b"])
    with pytest.raises(ValueError, match="num_hard_negatives"):
        TwoTowerModel([qf], [cf], "i", 8, device=CPU, num_hard_negatives=k)


def test_c_entries_refuse_bad_arguments():
    lib = _native.lib()
    bad = _native.TT_ERR_BAD_ARG
    p = 4096  # never dereferenced: every call below returns before a launch
    big = 1 << 30
    thr_fn, rows, cols, fused = (lib.tt_inbatch_hard_threshold, lib.tt_inbatch_xent_rows_hard,
                                 lib.tt_inbatch_xent_cols_hard, lib.tt_inbatch_softmax_xent_hard)
    assert thr_fn(p, 8, 4, p, 8, 4, 8, None, 0, None, None, 0, 0, p, p, big, None) == bad
    assert "k must be >= 1" in lib.tt_last_error().decode()
    assert thr_fn(p, 8, 4, p, 8, 4, 8, None, 0, None, None, 0, -3, p, p, big, None) == bad
    assert thr_fn(p, 8, 4, p, 8, 4, 8, None, 0, None, None, 0, 2, None, p, big, None) == bad
    assert "NULL thr" in lib.tt_last_error().decode()
    assert thr_fn(p, 8, 4, p, 8, 4, 8, None, 0, p, None, 0, 2, p, p, big, None) == bad  # one id vector only
    assert thr_fn(p, 8, 4, p, 8, 4, 8, None, 1, None, None, 0, 2, p, p, big, None) == bad  # positives past n_cols
    assert thr_fn(None, 8, 4, p, 8, 4, 8, None, 0, None, None, 0, 2, p, p, big, None) == bad
    assert thr_fn(p, 256, 4, p, 256, 4, 256, None, 0, None, None, 0, 2, p, p, big, None) == _native.TT_ERR_UNSUPPORTED
    assert thr_fn(p, 8, 4, p, 8, 4, 8, None, 0, None, None, 0, 2, p, p, 16, None) == _native.TT_ERR_WORKSPACE
    assert rows(p, 8, 4, p, 8, 4, 8, None, 0, None, None, 0, None, p, p, None, p, big, None) == bad
    assert "NULL thr" in lib.tt_last_error().decode()
    assert rows(p, 8, 4, p, 8, 4, 8, None, 0, p, None, 0, p, p, p, None, p, big, None) == bad
    assert rows(p, 8, 4, p, 8, 4, 8, None, 0, None, None, 0, p, p, p, None, p, 16, None) == _native.TT_ERR_WORKSPACE
    assert cols(p, 8, 4, p, None, p, 8, 4, 8, None, 0, None, None, 0, None, p, p, big, None) == bad
    assert "NULL thr" in lib.tt_last_error().decode()
    assert cols(p, 8, 4, p, None, p, 8, 4, 8, None, 0, None, None, 0, p, p, p, 16, None) == _native.TT_ERR_WORKSPACE
    assert fused(p, 8, p, 8, 4, 8, None, None, 0, 0, p, p, p, p, p, 1.0, None, p, big, None) == bad
    assert "k must be >= 1" in lib.tt_last_error().decode()
    assert fused(p, 8, p, 8, 4, 8, None, None, 0, 3, p, p, p, p, None, 1.0, None, p, big, None) == bad
    assert fused(p, 8, p, 8, 4, 8, None, None, 0, 3, p, p, p, p, p, 1.0, None, p, 16, None) == _native.TT_ERR_WORKSPACE
    # the workspaces: the hits ones plus the padded thresholds; 0 for an unsupported dim
    for x3 in (0, 1):
        assert lib.tt_inbatch_hard_workspace_size(200, 448, 64, x3) >= \
            lib.tt_inbatch_hits_workspace_size(200, 448, 64, x3) + 448 * 4
        assert lib.tt_inbatch_fused_hard_workspace_size(200, 64, x3) >= \
            lib.tt_inbatch_fused_hits_workspace_size(200, 64, x3) + 256 * 4
    assert lib.tt_inbatch_hard_workspace_size(16, 16, 300, 0) == 0
    assert lib.tt_inbatch_fused_hard_workspace_size(16, 300, 0) == 0
