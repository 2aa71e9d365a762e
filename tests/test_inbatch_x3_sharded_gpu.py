"""The fp32-faithful (x3) in-batch loss on the rank-sharded path: the
rectangular launches of the X3 pass kernel (tt_inbatch_xent_rows_x3 /
tt_inbatch_xent_cols_x3: stationary rows padded to 128 against streamed rows
padded to 64, pos_offset > 0, short and empty splits, fewer tiles per split
than ring stages) against torch fp64, against the fused x3 entry, and through
the data-parallel train step and the evaluation loss under TT_INBATCH_X3=1."""
import numpy as np
import pytest
import torch

from pkg.modelling import hip_ops

pytestmark = pytest.mark.gpu

# (G, B, E, scale): G ranks emulated on one device by slicing the batch
CASES = [
    (3, 384, 64, 2.0),     # b = 128: exact 128 padding, 6 streamed tiles, one per split
    (2, 200, 128, 1.5),    # b = 100: 28 padded stationary rows, 56 padded streamed rows (-inf bias); 129 KB LDS
    (4, 320, 37, 2.5),     # b = 80: odd dim (scalar prep loads), D padded to 64
    (1, 1, 16, 3.0),       # one row, pos_offset 0
    (4, 2080, 128, 1.5),   # b = 520: stat_pad 640, strm_pad 2112 = 33 tiles: 11 splits of 3 tiles, 5 empty
    (3, 384, 128, 1.5),    # b = 128 at D = 128 (the fourth shape of the bf16 drift measurements)
]
# (B, E, scale) the bf16 contract's drift from fp64 was measured on (CPU restatement,
# oracle.inbatch_softmax_xent_bf16): dQ 8.6e-3, 8.7e-3, 9.4e-3, 7.1e-3; dC 6.1e-3 .. 7.4e-3
BF16_DRIFTS = {(384, 64, 2.0), (384, 128, 1.5), (320, 37, 2.5), (200, 128, 1.5)}

_REF: dict = {}


def _inputs(cuda, B, E, scale):
    """The inputs of test_inbatch_x3_vs_torch_fp64 and their fp64 loss and
    gradients (torch on the device, blocked); computed once per shape."""
    key = (B, E, scale)
    if key in _REF:
        return _REF[key]
    g = torch.Generator(device=cuda)
    g.manual_seed(B + E)
    q = torch.relu(torch.randn(B, E, generator=g, device=cuda)) * scale
    c = torch.relu(torch.randn(B, E, generator=g, device=cuda)) * scale
    c[::3] = q[::3] * 0.9  # confident positives
    logq = torch.log(torch.rand(B, generator=g, device=cuda) * 1e-3 + 1e-6)
    qd, cd, ld = q.double(), c.double(), logq.double()
    dq_ref = torch.empty_like(qd)
    dc_ref = torch.zeros_like(cd)
    rl = torch.empty(B, dtype=torch.float64, device=cuda)
    for s0 in range(0, B, 2048):
        S = qd[s0:s0 + 2048] @ cd.T - ld[None, :]
        lse_ref = torch.logsumexp(S, 1)
        r = torch.arange(s0, min(s0 + 2048, B), device=cuda)
        rl[s0:s0 + 2048] = lse_ref - S[r - s0, r]
        P = torch.exp(S - lse_ref[:, None])
        P[r - s0, r] -= 1.0
        dq_ref[s0:s0 + 2048] = P @ cd
        dc_ref += P.T @ qd[s0:s0 + 2048]
    _REF[key] = (q, c, logq, float(rl.sum()), dq_ref, dc_ref)
    return _REF[key]


def _sharded(q, c, logq, G, x3):
    """Every emulated rank's rows pass, the gather of lse and row_loss, then
    every rank's cols pass: (row_loss [B], dq [B, E], dc [B, E])."""
    B = q.shape[0]
    b = B // G
    assert b * G == B
    rows = [hip_ops.inbatch_rows(q[r * b:(r + 1) * b], c, logq, pos_offset=r * b, x3=x3) for r in range(G)]
    lse_all = torch.cat([o[0] for o in rows])
    loss_all = torch.cat([o[1] for o in rows])
    dq = torch.cat([o[2] for o in rows])
    dc = torch.cat([hip_ops.inbatch_cols(q, lse_all, c[r * b:(r + 1) * b], logq[r * b:(r + 1) * b], pos_offset=r * b,
                                         row_loss=loss_all, x3=x3) for r in range(G)])
    return lse_all, loss_all, dq, dc


def _rel(x, ref):
    return float((x.double() - ref).norm() / ref.norm().clamp_min(1e-30))


@pytest.mark.parametrize("G,B,E,scale", CASES)
def test_sharded_x3_vs_torch_fp64(cuda, G, B, E, scale):
    """rows + cols with x3=True over G emulated ranks hold the project's x3
    bounds against fp64 (loss 1e-4, dQ and dC 1e-3 relative in norm); on the
    same tensors the bf16 entries do not hold 1e-3, so a dropped flag fails."""
    q, c, logq, loss_ref, dq_ref, dc_ref = _inputs(cuda, B, E, scale)
    lse, row_loss, dq, dc = _sharded(q, c, logq, G, x3=True)
    loss = float(row_loss.double().sum())
    e_dq, e_dc = _rel(dq, dq_ref), _rel(dc, dc_ref)
    print(f"x3 G={G} B={B} E={E}: loss {loss:.9g} ref {loss_ref:.9g}, dq {e_dq:.3e}, dc {e_dc:.3e}")
    for t in (lse, row_loss, dq, dc):
        assert bool(torch.isfinite(t).all())
    assert abs(loss - loss_ref) <= 1e-4 * abs(loss_ref) + 1e-6
    assert e_dq <= 1e-3
    assert e_dc <= 1e-3
    if (B, E, scale) in BF16_DRIFTS:
        _, _, dq16, dc16 = _sharded(q, c, logq, G, x3=False)
        b_dq, b_dc = _rel(dq16, dq_ref), _rel(dc16, dc_ref)
        print(f"bf16 G={G} B={B} E={E}: dq {b_dq:.3e}, dc {b_dc:.3e}")
        assert max(b_dq, b_dc) > 1e-3


@pytest.mark.parametrize("G,B,E,scale", [(2, 200, 128, 1.5), (4, 2080, 128, 1.5)])
def test_sharded_x3_rows_without_dq(cuda, G, B, E, scale):
    """want_dq=False (the evaluation loss's call) changes nothing else."""
    q, c, logq = _inputs(cuda, B, E, scale)[:3]
    b = B // G
    r = G - 1
    lse, rl, dq = hip_ops.inbatch_rows(q[r * b:], c, logq, pos_offset=r * b, x3=True)
    lse2, rl2, none = hip_ops.inbatch_rows(q[r * b:], c, logq, pos_offset=r * b, want_dq=False, x3=True)
    assert none is None and dq is not None
    assert torch.equal(lse, lse2) and torch.equal(rl, rl2)


@pytest.mark.parametrize("B,E,scale", [(384, 64, 2.0), (2048, 128, 1.5)])
def test_sharded_x3_equals_fused_x3_at_one_rank(cuda, B, E, scale):
    """At G = 1 the rows + cols entries and the fused x3 entry plan alike
    (same padding, split and combines), so they differ at most in fp32
    summation order: rtol 1e-5, atol 1e-6 max|ref|."""
    q, c, logq = _inputs(cuda, B, E, scale)[:3]
    got = _sharded(q, c, logq, 1, x3=True)
    want = hip_ops.inbatch_fused(q, c, logq, x3=True)
    names = ("lse", "row_loss", "dq", "dc")
    print(f"B={B} E={E} bit-equal:", {n: bool(torch.equal(g, w)) for n, g, w in zip(names, got, want)})
    for n, g, w in zip(names, got, want):
        assert torch.allclose(g, w, rtol=1e-5, atol=1e-6 * float(w.abs().max())), n


def test_eval_loss_matches_the_fused_x3_loss(cuda, monkeypatch):
    """Under TT_INBATCH_X3=1 the no-grad loss is computed from the scores the
    training loss is computed from."""
    from pkg.modelling.losses import inbatch_softmax_xent

    monkeypatch.setenv("TT_INBATCH_X3", "1")
    q, c, logq = _inputs(cuda, 384, 64, 2.0)[:3]
    assert not q.requires_grad and not c.requires_grad
    got = inbatch_softmax_xent(q, c, logq)
    want = hip_ops.inbatch_fused(q, c, logq, x3=True, loss_scale=1.0)[4]
    torch.testing.assert_close(got, want, rtol=1e-6, atol=0)


def test_x3_sharded_step_world2_matches_full_batch(cuda, monkeypatch):
    """test_global_negatives_sharded_step_matches_full_batch at world 2 with
    TT_INBATCH_X3=1 on both sides (the spawned ranks inherit it): the ranks run
    the x3 rows / cols entries, the single-GPU model the fused x3 entry; both
    are x3 arithmetic and differ only in fp32 summation order, so that test's
    per-step restart scheme, tolerances and their derivation carry over."""
    import torch.multiprocessing as mp

    from test_distributed_gpu import _free_port, _global_batches, _load_state, _small_model, _step_worker

    monkeypatch.setenv("TT_INBATCH_X3", "1")
    world, steps = 2, 3
    batches = _global_batches(steps, 64 * world)
    out = mp.Manager().dict()
    mp.spawn(_step_worker, args=(world, _free_port(), batches, out), nprocs=world, join=True)
    losses0, states0 = out[0]
    losses1, states1 = out[1]
    assert losses1 == losses0
    for (fa, ta), (fb, tb) in zip(states1, states0):
        assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(fa, fb))
        assert all(np.array_equal(ta[k][0], tb[k][0]) and np.array_equal(ta[k][1], tb[k][1]) for k in ta)
    ref = _small_model(cuda, 3)
    for s, gb in enumerate(batches):
        _load_state(ref, states0[s])
        ref_loss = float(ref.train_step({k: torch.as_tensor(v, device=cuda) for k, v in gb.items()})["loss"].item())
        np.testing.assert_allclose(losses0[s], ref_loss, rtol=2e-5)
        flats, tables = states0[s + 1]
        opt = ref.optimizer
        for ti, t in enumerate(ref.towers):
            np.testing.assert_allclose(flats[ti][0], t.dense.flat.detach().cpu().numpy(), rtol=0, atol=2e-6)
            np.testing.assert_allclose(flats[ti][1], opt._slots[id(t.dense.flat)][0].cpu().numpy(), rtol=1e-5)
            for name, e in t.input_layer.embedding_layers.items():
                np.testing.assert_allclose(tables[(ti, name)][0], e.weight.cpu().numpy(), rtol=0, atol=2e-6)
                np.testing.assert_allclose(tables[(ti, name)][1], opt._slots[id(e.weight)][0].cpu().numpy(),
                                           rtol=1e-5)


def test_x3_sharded_step_world1_captured(cuda, monkeypatch):
    """Under TT_INBATCH_X3=1 the world-1 global-negatives step (the fused x3
    entry inside its captured graph) trains bit-identically to the single-GPU
    train step, as the bf16 pair does; the same step with its collectives
    forced (BatchComm(always=True): the x3 rows / cols entries, captured)
    follows it within the summation-order tolerances of the world-2 test
    (2e-6 per step on parameters, 2e-5 on the loss)."""
    import socket

    import torch.distributed as dist

    from pkg.modelling.distributed import BatchComm, ShardedTrainStep, destroy_process_group
    from pkg.modelling.models.two_tower_model import GraphedTrainStep
    from test_model_gpu import _batch, _small_model

    monkeypatch.setenv("TT_INBATCH_X3", "1")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device(cuda))
    try:
        a, b, c = (_small_model(cuda, seed=8) for _ in range(3))
        short = ShardedTrainStep(a, shard_min_rows=300, global_negatives=True)
        split = ShardedTrainStep(b, shard_min_rows=300, global_negatives=True, comm=BatchComm(always=True))
        assert short.use_graph and split.use_graph
        rng = np.random.default_rng(17)
        steps = 3  # call 1 eager, call 2 captures and replays, call 3 replays
        batches = [_batch(cuda, rng, 256) for _ in range(steps)]
        single = GraphedTrainStep(c, batches[0], warmup=1)  # its warm-up step trains on batch 0
        for i, batch in enumerate(batches):
            la, lb = short(batch)["loss"], split(batch)["loss"]
            lc = single.warmup_out["loss"] if i == 0 else single(batch)["loss"]
            assert torch.equal(la, lc), (i, la, lc)
            torch.testing.assert_close(lb, la, rtol=2e-5 * (i + 1), atol=0)
        assert short._graph is not None and split._graph is not None
        for ta, tb, tc in zip(a.towers, b.towers, c.towers):
            assert torch.equal(ta.dense.flat, tc.dense.flat)
            torch.testing.assert_close(tb.dense.flat, ta.dense.flat, rtol=0, atol=2e-6 * steps)
            for name, t in tc.input_layer.embedding_layers.items():
                ma, mb = ta.input_layer.embedding_layers[name], tb.input_layer.embedding_layers[name]
                ga = short.tables.gather_full(ma._shard_key) if hasattr(ma, "_shard_key") else ma.weight
                gb = split.tables.gather_full(mb._shard_key) if hasattr(mb, "_shard_key") else mb.weight
                assert torch.equal(ga, t.weight), name
                torch.testing.assert_close(gb, ga, rtol=0, atol=2e-6 * steps)
        short.check_status()
        split.check_status()
    finally:
        destroy_process_group()  # the captured step graphs first, then the group
