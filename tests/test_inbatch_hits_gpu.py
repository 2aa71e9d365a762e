"""Opt-in removal of accidental hits from the in-batch loss (duplicate
candidates in the batch are no negatives of their own rows): the HITS form of
the pass kernel through tt_inbatch_softmax_xent_hits, tt_inbatch_xent_rows_hits
and tt_inbatch_xent_cols_hits, bf16 and x3, against torch fp64 of the masked
loss, against the plain entries (bit for bit with distinct ids), and through
TwoTowerModel(remove_accidental_hits=True).

Inputs: Zipf candidate ids over V articles, candidates gathered from one
embedding table (so equal ids have equal embeddings and S_ij == S_ii for every
copy j of row i's article), every second query a confident positive, and the
empirical logQ of the batch.  On these inputs the masked and the unmasked fp64
losses differ by 1.3-25 % and their dC by 9e-2 .. 4e-1 relative in norm, one
to two orders above every tolerance below: an entry that ignores its ids
fails."""
import numpy as np
import pytest
import torch

import inbatch_rowwise
from oracle import oracle
from pkg.modelling import hip_ops

pytestmark = pytest.mark.gpu

# (B, E, V, scale); max|S| <= 16, the regime of the bf16 tolerances (tests/test_kernels_gpu.py)
BF16_CASES = [(64, 16, 8, 1.0), (129, 100, 40, 0.5), (300, 64, 60, 0.5), (1024, 128, 200, 0.3)]
# trained score magnitudes: the x3 tolerances' regime
X3_CASES = [(384, 64, 50, 2.0), (2080, 128, 400, 1.5), (1, 16, 1, 3.0)]
# (G, B, E, V, scale): G ranks emulated on one device.  The shapes of the x3
# sharded test (padded stationary and streamed rows, pos_offset > 0, empty
# splits, fewer tiles than ring stages), at scales where max|S| <= 16 so that
# the bf16 and the x3 tolerances both apply to the same reference.
RECT_CASES = [(2, 200, 128, 40, 0.3), (3, 384, 64, 50, 0.5), (4, 320, 37, 60, 0.5), (4, 2080, 128, 400, 0.3)]
BF16_TOL = (1e-3, 1e-2, 1e-2)  # loss (relative), dq, dc (relative in norm)
X3_TOL = (1e-4, 1e-3, 1e-3)

_REF: dict = {}


def _masked_fp64(q, c, logq, ids):
    """torch fp64 of the masked loss (include/tt.h), blocked over rows:
    (row_loss [B], dq, dc); ids None: the reference's unmasked loss."""
    dev = q.device
    B = q.shape[0]
    qd, cd, ld = q.double(), c.double(), logq.double()
    dq_ref = torch.empty_like(qd)
    dc_ref = torch.zeros_like(cd)
    rl = torch.empty(B, dtype=torch.float64, device=dev)
    for s0 in range(0, B, 2048):
        r = torch.arange(s0, min(s0 + 2048, B), device=dev)
        S = qd[r] @ cd.T - ld[None, :]
        if ids is not None:
            hit = ids[r][:, None] == ids[None, :]
            hit[r - s0, r] = False
            S = S.masked_fill(hit, float("-inf"))
        lse = torch.logsumexp(S, 1)
        rl[r] = lse - S[r - s0, r]
        P = torch.exp(S - lse[:, None])
        P[r - s0, r] -= 1.0
        dq_ref[r] = P @ cd
        dc_ref += P.T @ qd[r]
    return rl, dq_ref, dc_ref


def _inputs(cuda, B, E, V, scale):
    """The recipe's tensors and their masked fp64 reference, once per shape:
    (q, c, logq, ids, loss_ref, dq_ref, dc_ref)."""
    key = (B, E, V, scale)
    if key in _REF:
        return _REF[key]
    ids_np = (np.random.default_rng(B + E).zipf(1.1, B) - 1) % V
    g = torch.Generator()
    g.manual_seed(B + E)
    table = torch.relu(torch.randn(V, E, generator=g)) * scale
    ids_cpu = torch.from_numpy(ids_np.astype(np.int64))
    c = table[ids_cpu]
    q = torch.relu(torch.randn(B, E, generator=g)) * scale
    q[::2] = 0.9 * c[::2]
    count = torch.bincount(ids_cpu, minlength=V).double()
    logq = torch.log(count / B)[ids_cpu].float()
    q, c, logq = q.to(cuda).contiguous(), c.to(cuda).contiguous(), logq.to(cuda)
    ids = ids_cpu.to(torch.int32).to(cuda)
    rl, dq_ref, dc_ref = _masked_fp64(q, c, logq, ids)
    _REF[key] = (q, c, logq, ids, float(rl.sum()), dq_ref, dc_ref)
    return _REF[key]


def _rel(x, ref):
    return float((x.double() - ref).norm() / ref.norm().clamp_min(1e-30))


def _sharded(q, c, logq, ids, G, x3):
    """Every emulated rank's rows pass, the gather of lse and row_loss, then
    every rank's cols pass: (lse [B], row_loss [B], dq [B, E], dc [B, E]).
    ids None: the plain entries."""
    B = q.shape[0]
    b = B // G
    assert b * G == B
    sl = [slice(r * b, (r + 1) * b) for r in range(G)]
    rk = lambda s: {} if ids is None else {"row_ids": ids[s], "col_ids": ids}  # noqa: E731
    ck = lambda s: {} if ids is None else {"row_ids": ids, "col_ids": ids[s]}  # noqa: E731
    rows = [hip_ops.inbatch_rows(q[s], c, logq, pos_offset=s.start, x3=x3, **rk(s)) for s in sl]
    lse_all = torch.cat([o[0] for o in rows])
    loss_all = torch.cat([o[1] for o in rows])
    dq = torch.cat([o[2] for o in rows])
    dc = torch.cat([hip_ops.inbatch_cols(q, lse_all, c[s], logq[s], pos_offset=s.start, row_loss=loss_all, x3=x3,
                                         **ck(s)) for s in sl])
    return lse_all, loss_all, dq, dc


def _errors(tag, out, loss_ref, dq_ref, dc_ref):
    lse, row_loss, dq, dc = out[:4]
    for t in (lse, row_loss, dq, dc):
        assert bool(torch.isfinite(t).all()), tag
    loss = float(row_loss.double().sum())
    e = (abs(loss - loss_ref) / max(abs(loss_ref), 1e-30) if loss_ref != 0.0 else abs(loss),
         _rel(dq, dq_ref) if float(dq_ref.norm()) > 0 else float(dq.abs().max()),
         _rel(dc, dc_ref) if float(dc_ref.norm()) > 0 else float(dc.abs().max()))
    print(f"{tag}: loss {loss:.9g} ref {loss_ref:.9g} ({e[0]:.3e}), dq {e[1]:.3e}, dc {e[2]:.3e}")
    return e


def _holds(e, tol):
    return e[0] <= tol[0] and e[1] <= tol[1] and e[2] <= tol[2]


def _check_vs_fp64(cuda, B, E, V, scale, x3, tol):
    q, c, logq, ids, loss_ref, dq_ref, dc_ref = _inputs(cuda, B, E, V, scale)
    tag = f"{'x3' if x3 else 'bf16'} B={B} E={E} V={V}"
    fused, sharded = hip_ops.inbatch_fused(q, c, logq, x3=x3, ids=ids), _sharded(q, c, logq, ids, 1, x3)
    e = _errors(tag + " fused hits", fused, loss_ref, dq_ref, dc_ref)
    assert _holds(e, tol), e
    e = _errors(tag + " rows+cols hits", sharded, loss_ref, dq_ref, dc_ref)
    assert _holds(e, tol), e
    # every element within its own bound (DESIGN.md §6 "Per-element guarantees")
    ids_np = ids.cpu().numpy()
    con = None if x3 else oracle.inbatch_softmax_xent_bf16(q.cpu().numpy(), c.cpu().numpy(), logq.cpu().numpy(),
                                                           row_ids=ids_np, col_ids=ids_np, aux=True)
    for name, out in (("fused", fused), ("rows+cols", sharded)):
        bad = (inbatch_rowwise.check_x3(out, q, c, logq, ids, f"{tag} {name}") if x3 else
               inbatch_rowwise.check_bf16(out, q, c, logq, con, ids, f"{tag} {name}"))
        assert not bad, "\n".join(bad)
    if len(torch.unique(ids)) < B:
        # the plain entry on the same tensors scores the duplicates as negatives
        e = _errors(tag + " fused plain", hip_ops.inbatch_fused(q, c, logq, x3=x3), loss_ref, dq_ref, dc_ref)
        assert not _holds(e, tol), e
        assert e[2] > 5 * tol[2], e


@pytest.mark.parametrize("B,E,V,scale", BF16_CASES)
def test_hits_bf16_vs_torch_fp64(cuda, B, E, V, scale):
    """The bf16 hits entries hold the bf16 path's own tolerances against the
    masked fp64 loss (loss 1e-3, dq and dc 1e-2 in norm); the plain entry on
    the same tensors does not (measured differences, masked vs unmasked fp64:
    loss 25 / 18 / 8 / 1.3 %, dC 0.41 / 0.38 / 0.28 / 0.093)."""
    _check_vs_fp64(cuda, B, E, V, scale, False, BF16_TOL)


@pytest.mark.parametrize("B,E,V,scale", X3_CASES)
def test_hits_x3_vs_torch_fp64(cuda, B, E, V, scale):
    """The x3 hits entries hold the x3 tolerances (loss 1e-4, dq and dc 1e-3);
    the plain x3 entry does not (masked vs unmasked fp64: loss 6 / 6.5 %, dC
    0.33 / 0.34).  B = 1: a single row, nothing to mask."""
    _check_vs_fp64(cuda, B, E, V, scale, True, X3_TOL)


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
@pytest.mark.parametrize("G,B,E,V,scale", RECT_CASES)
def test_hits_rectangular_launches(cuda, G, B, E, V, scale, x3):
    """rows + cols with ids over G emulated ranks (each rank's rows against
    the gathered columns' ids, the gathered rows' ids against its columns)."""
    q, c, logq, ids, loss_ref, dq_ref, dc_ref = _inputs(cuda, B, E, V, scale)
    tol = X3_TOL if x3 else BF16_TOL
    e = _errors(f"{'x3' if x3 else 'bf16'} G={G} B={B} E={E}", _sharded(q, c, logq, ids, G, x3), loss_ref, dq_ref,
                dc_ref)
    assert _holds(e, tol), e
    e = _errors(f"plain G={G} B={B} E={E}", _sharded(q, c, logq, None, G, x3), loss_ref, dq_ref, dc_ref)
    assert not _holds(e, tol), e


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
def test_hits_more_tiles_per_split_than_ring_stages(cuda, x3):
    """B = 8192: 64 stationary blocks -> 8 splits of 16 streamed tiles, so
    every stage of the 4-deep ring, its id slot included, is refilled three
    times while the pass runs (the shapes above stream at most 3 tiles per
    split).  A miscounted wait would read a stale stage's ids: wrong masks.
    Against fp64 at max|S| <= 16 (both tolerances apply), and bit for bit
    against the plain entry with distinct ids."""
    B, E, V, scale = 8192, 128, 2000, 0.3
    q, c, logq, ids, loss_ref, dq_ref, dc_ref = _inputs(cuda, B, E, V, scale)
    tol = X3_TOL if x3 else BF16_TOL
    e = _errors(f"{'x3' if x3 else 'bf16'} B={B} fused hits", hip_ops.inbatch_fused(q, c, logq, x3=x3, ids=ids),
                loss_ref, dq_ref, dc_ref)
    assert _holds(e, tol), e
    plain = hip_ops.inbatch_fused(q, c, logq, x3=x3)
    e = _errors(f"{'x3' if x3 else 'bf16'} B={B} fused plain", plain, loss_ref, dq_ref, dc_ref)
    assert not _holds(e, tol), e
    distinct = torch.arange(B, dtype=torch.int32, device=cuda)
    for n, a, b in zip(("lse", "row_loss", "dq", "dc"), hip_ops.inbatch_fused(q, c, logq, x3=x3, ids=distinct), plain):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
@pytest.mark.parametrize("B,E,V,scale", [(384, 64, 50, 0.5), (2080, 128, 400, 0.3)])
def test_hits_rows_cols_equal_fused_at_one_rank(cuda, B, E, V, scale, x3):
    """At G = 1 the rows + cols hits entries and the fused hits entry plan
    alike, so they differ at most in fp32 summation order: the bounds of
    test_sharded_x3_equals_fused_x3_at_one_rank (rtol 1e-5, atol 1e-6 max|ref|)."""
    q, c, logq, ids = _inputs(cuda, B, E, V, scale)[:4]
    got = _sharded(q, c, logq, ids, 1, x3)
    want = hip_ops.inbatch_fused(q, c, logq, x3=x3, ids=ids)
    for n, g, w in zip(("lse", "row_loss", "dq", "dc"), got, want):
        assert torch.allclose(g, w, rtol=1e-5, atol=1e-6 * float(w.abs().max())), n


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
@pytest.mark.parametrize("B,E", [(1, 16), (37, 37), (129, 100), (2080, 128)])
def test_hits_distinct_ids_equal_plain_bit_for_bit(cuda, B, E, x3):
    """With pairwise distinct ids nothing is masked: every select takes the
    bias, so every hits entry returns the plain entry's bits."""
    g = torch.Generator(device=cuda)
    g.manual_seed(B + E)
    q = torch.randn(B, E, generator=g, device=cuda)
    c = torch.randn(B, E, generator=g, device=cuda)
    logq = torch.log(torch.rand(B, generator=g, device=cuda) * 1e-3 + 1e-6)
    ids = torch.arange(B, dtype=torch.int32, device=cuda)
    for n, a, b in zip(("lse", "row_loss", "dq", "dc"), hip_ops.inbatch_fused(q, c, logq, x3=x3, ids=ids),
                       hip_ops.inbatch_fused(q, c, logq, x3=x3)):
        assert torch.equal(a, b), ("fused", n)
    la, ra, dqa = hip_ops.inbatch_rows(q, c, logq, x3=x3, row_ids=ids, col_ids=ids)
    lb, rb, dqb = hip_ops.inbatch_rows(q, c, logq, x3=x3)
    assert torch.equal(la, lb) and torch.equal(ra, rb) and torch.equal(dqa, dqb)
    dca = hip_ops.inbatch_cols(q, la, c, logq, row_loss=ra, x3=x3, row_ids=ids, col_ids=ids)
    dcb = hip_ops.inbatch_cols(q, lb, c, logq, row_loss=rb, x3=x3)
    assert torch.equal(dca, dcb)


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
@pytest.mark.parametrize("B,E", [(37, 37), (300, 128)])
def test_hits_all_ids_equal_is_exactly_zero(cuda, B, E, x3):
    """Every other column a hit: lse_neg = -inf, so each row's loss and dq row
    are exactly 0 and nothing reaches any dc; all outputs finite."""
    g = torch.Generator(device=cuda)
    g.manual_seed(B)
    q = torch.randn(B, E, generator=g, device=cuda)
    c = torch.randn(B, E, generator=g, device=cuda)
    logq = torch.log(torch.rand(B, generator=g, device=cuda) * 1e-3 + 1e-6)
    ids = torch.full((B,), 7, dtype=torch.int32, device=cuda)
    for out in (hip_ops.inbatch_fused(q, c, logq, x3=x3, ids=ids, loss_scale=1.0), _sharded(q, c, logq, ids, 1, x3)):
        lse, row_loss, dq, dc = out[:4]
        assert bool(torch.isfinite(lse).all())
        for t in (row_loss, dq, dc) + tuple(out[4:]):
            assert bool((t == 0).all())


@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
def test_hits_across_tile_and_split_boundaries(cuda, x3):
    """Row 5's article again at columns 63 and 64 (either side of the first
    64-row tile boundary) and at column 192, the first column of the second
    split (B = 2080: 2176 padded rows, 17 stationary blocks -> 16 splits of
    192 streamed rows, in the fused plan and in the rows / cols plans alike);
    every other id distinct.  Small scores (max|S| <= 16), so the bf16
    tolerances apply as well.  The four rows are confident (their positive's
    score is about the lse of their ~2000 true negatives), so one unmasked
    copy, whose score equals the positive's, moves lse_neg by
    log(1 + e^(pos - lse_neg)) = O(1): the four rows are also checked on
    their own, each row's loss to the gradients' tolerance (a single row's
    loss has none of the batch sum's averaging)."""
    B, E = 2080, 128
    g = torch.Generator(device=cuda)
    g.manual_seed(5)
    q = torch.relu(torch.randn(B, E, generator=g, device=cuda)) * 0.3
    c = torch.relu(torch.randn(B, E, generator=g, device=cuda)) * 0.3
    dup = [5, 63, 64, 192]
    c[dup] = 1.6 * c[5]
    q[dup] = 0.9 * c[5]  # the copies would be each other's strongest negatives
    ids = torch.arange(B, dtype=torch.int32, device=cuda)
    ids[dup] = 5
    logq = torch.log(torch.rand(B, generator=g, device=cuda) * 0.5 + 0.5)
    rl, dq_ref, dc_ref = _masked_fp64(q, c, logq, ids)
    tol = X3_TOL if x3 else BF16_TOL
    d = torch.tensor(dup, device=cuda)
    for tag, out in (("fused", hip_ops.inbatch_fused(q, c, logq, x3=x3, ids=ids)),
                     ("rows+cols", _sharded(q, c, logq, ids, 1, x3)),
                     ("G=4", _sharded(q, c, logq, ids, 4, x3))):
        e = _errors(f"boundaries {tag}", out, float(rl.sum()), dq_ref, dc_ref)
        assert _holds(e, tol), e
        # the four rows themselves (a missed mask is invisible in the whole batch's norm)
        e4 = (float(((out[1][d].double() - rl[d]) / rl[d]).abs().max()), _rel(out[2][d], dq_ref[d]),
              _rel(out[3][d], dc_ref[d]))
        print(f"boundaries {tag} rows {dup}: {e4}")
        assert _holds(e4, (tol[1], tol[1], tol[2])), e4
    plain = hip_ops.inbatch_fused(q, c, logq, x3=x3)
    assert _rel(plain[3][d], dc_ref[d]) > 5 * tol[2]


# --------------------------------------------------------------------------- model level
def _hits_model(cuda, seed, hits=True):
    """tests/test_model_gpu.py's small model, with the flag."""
    from pkg import dtypes
    from pkg.modelling.models.two_tower_model import TwoTowerModel
    from pkg.modelling.optimizer_factory import OptimizerFactory
    from pkg.schema.features import Feature, FeatureFamily

    V = [str(i) for i in range(300)]
    qf = [Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=16, vocab=V),
          Feature("post", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V[:50])]
    cf = [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=16, vocab=V),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=V[:20]),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=4, vocab=V[:20])]
    probs = {str(i): float(p) for i, p in enumerate(np.random.default_rng(seed).dirichlet(np.ones(300)))}
    m = TwoTowerModel(qf, cf, "art", 32, [64], [64], probs, device=cuda, seed=seed, remove_accidental_hits=hits)
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", {"learning_rate": 0.05}))
    return m


def _same_state(a, b):
    for ta, tb in zip(a.towers, b.towers):
        assert torch.equal(ta.dense.flat, tb.dense.flat)
        for n in ta.input_layer.embedding_layers:
            assert torch.equal(ta.input_layer.embedding_layers[n].weight, tb.input_layer.embedding_layers[n].weight)


def test_model_flag_eager_graphed_and_loss_level(cuda, tmp_path):
    """remove_accidental_hits=True: three eager steps and the graphed step
    (its warm-up step, then two replays: the ids are a view of the static
    word buffer) give bit-identical losses and parameters; the first step's
    loss is the loss-level entry's on the model's own tower outputs and ids;
    the flag-off model's loss on the same batch (Zipf ids: duplicates)
    differs; evaluation masks as training does; the flag survives save/load."""
    from pkg.modelling.losses import inbatch_softmax_xent
    from pkg.modelling.models.two_tower_model import GraphedTrainStep, TwoTowerModel
    from test_model_gpu import _batch

    a, b, off = _hits_model(cuda, 5), _hits_model(cuda, 5), _hits_model(cuda, 5, hits=False)
    rng = np.random.default_rng(11)
    batches = [_batch(cuda, rng, 256) for _ in range(3)]
    x = batches[0]
    assert len(torch.unique(x["art"])) < 256
    with torch.no_grad():
        qc, cc = a._split(x)
        qe, ce = a.query_tower.call(qc), a.candidate_tower.call(cc)
        logq = a.candidate_logq(x)
        want = inbatch_softmax_xent(qe, ce, logq, ids=x["art"])
        plain = inbatch_softmax_xent(qe, ce, logq)
        # evaluation takes the ids too (same tower outputs up to the MLP launches' fp32 summation order)
        torch.testing.assert_close(a.compute_loss(x, training=False), want, rtol=1e-5, atol=0)
    fused = hip_ops.inbatch_fused(qe, ce, logq, ids=x["art"], loss_scale=1.0)[4]
    eager = [a.train_step(bt)["loss"] for bt in batches]
    torch.testing.assert_close(eager[0], fused, rtol=1e-5, atol=0)
    # the no-grad rows entry sums the same row losses (bf16 contract either way)
    torch.testing.assert_close(want, fused, rtol=1e-5, atol=0)
    l_off = off.train_step(x)["loss"]
    print(f"model loss: hits {float(eager[0]):.6f}, plain {float(l_off):.6f}")
    torch.testing.assert_close(l_off, plain, rtol=1e-5, atol=0)
    assert abs(float(l_off) - float(eager[0])) > 1e-3 * abs(float(eager[0]))
    g = GraphedTrainStep(b, batches[0], warmup=1)
    graphed = [g.warmup_out["loss"].clone()] + [g(bt)["loss"].clone() for bt in batches[1:]]
    torch.cuda.synchronize()
    for le, lg in zip(eager, graphed):
        assert torch.equal(le, lg)
    _same_state(a, b)
    path = str(tmp_path / "m" / "two_tower")
    a.save(path)
    assert TwoTowerModel.load(path, device=cuda).remove_accidental_hits is True
    off.save(path)
    assert TwoTowerModel.load(path, device=cuda).remove_accidental_hits is False


@pytest.mark.parametrize("global_negatives", [False, True])
def test_sharded_world1_with_flag_matches_single_gpu(cuda, global_negatives):
    """A world-1 ShardedTrainStep of a flagged model gives the single-device
    step's losses and parameters, bit for bit as
    test_sharded_train_step_world1_matches_single_gpu asserts without it."""
    import socket

    import torch.distributed as dist

    from pkg.modelling.distributed import ShardedTrainStep, destroy_process_group
    from test_model_gpu import _batch

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device(cuda))
    try:
        a, b, off = _hits_model(cuda, 3), _hits_model(cuda, 3), _hits_model(cuda, 3, hits=False)
        step = ShardedTrainStep(a, shard_min_rows=300, global_negatives=global_negatives)
        rng = np.random.default_rng(7)
        batches = [_batch(cuda, rng, 256) for _ in range(3)]  # call 1 eager, 2 captures and replays, 3 replays
        for i, batch in enumerate(batches):
            la = step(batch)["loss"]
            lb = b.train_step(batch)["loss"]
            assert torch.equal(la, lb), (i, la, lb)
            if i == 0:
                assert not torch.equal(la, off.train_step(batch)["loss"])
        for ta, tb in zip(a.towers, b.towers):
            assert torch.equal(ta.dense.flat, tb.dense.flat)
            for name, t in tb.input_layer.embedding_layers.items():
                mine = ta.input_layer.embedding_layers[name]
                full = step.tables.gather_full(mine._shard_key) if hasattr(mine, "_shard_key") else mine.weight
                assert torch.equal(full, t.weight), name
    finally:
        destroy_process_group()  # the captured step graphs first, then the group
