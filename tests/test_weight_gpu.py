"""GPU: per-example sample weights — tt_inbatch_weight_rows' contract row by
row, its two libm outputs against fp64, the weighted loss and gradients
against fp64 autograd (x3 and default arithmetic, with and without accidental
hits), the structural identities (all weights 1, weight-0 rows, weights=None)
and the model's weighted step on every path.

The fold's outputs are views of a Workspace buffer that the next call
overwrites, so every result kept across calls is cloned."""
import numpy as np
import pytest
import torch

import weight_ref
from pkg import _native, dtypes
from pkg.modelling import hip_ops, losses
from pkg.modelling.dataset import DeviceDataset, EncodedDataset
from pkg.modelling.models import two_tower_model
from pkg.modelling.models.two_tower_model import WEIGHT_KEY, GraphedTrainStep, TwoTowerModel
from pkg.modelling.optimizer_factory import OptimizerFactory
from pkg.schema.features import Feature, FeatureFamily

pytestmark = pytest.mark.gpu

U = 2.0 ** -23


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _dq_views(cuda, n, dim, rng):
    """The same [n, dim] values twice: rows 16-byte aligned with a leading
    dimension that is a multiple of 4, and (the scalar path) an odd leading
    dimension from a base 4 bytes past an aligned address.  Columns past dim
    hold a sentinel."""
    vals = torch.as_tensor(rng.standard_normal((n, dim)).astype(np.float32), device=cuda)
    ld_a = (dim + 3) // 4 * 4 + 4
    ld_s = ld_a + 1
    a = torch.full((n, ld_a), 777.0, device=cuda)
    s_buf = torch.full((n * ld_s + 1,), 777.0, device=cuda)
    s = s_buf[1:].view(n, ld_s)
    a[:, :dim] = vals
    s[:, :dim] = vals
    assert a.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 4 and s.stride(0) % 2 == 1
    return vals, a, s


def _weights(n, rng):
    """Weights inside (0, 1) with ones and zeros at fixed places (every fifth row each)."""
    w = rng.uniform(0.01, 0.99, n).astype(np.float32)
    w[0::5] = 1.0
    w[2::5] = 0.0
    if n == 1:
        w[0] = 0.375
    return w


@pytest.mark.parametrize("dim", [1, 4, 100, 128, 300])
@pytest.mark.parametrize("n", [1, 63, 64, 257])
def test_kernel_contract(cuda, n, dim):
    rng = np.random.default_rng(1000 * n + dim)
    w = _weights(n, rng)
    lse = rng.uniform(-5, 12, n).astype(np.float32)
    rl = np.exp(rng.uniform(np.log(1e-4), np.log(40.0), n)).astype(np.float32)
    vals, dq_a, dq_s = _dq_views(cuda, n, dim, rng)
    zero = torch.as_tensor(w == 0, device=cuda)
    for d in (dq_a, dq_s):  # an inf / NaN in a weight-0 row must not survive
        d[:, :dim][zero] = float("nan")
        if dim > 1:
            d[:, 1:dim][zero] = float("inf")
    tw, tl, tr = (torch.as_tensor(x, device=cuda) for x in (w, lse, rl))
    before = dq_a[:, :dim].clone()
    out_a = [t.clone() for t in hip_ops.inbatch_weight_rows(tw, tl, tr, dq_a[:, :dim])]
    out_s = [t.clone() for t in hip_ops.inbatch_weight_rows(tw, tl, tr, dq_s[:, :dim])]
    torch.cuda.synchronize()
    # the aligned and the scalar path: the same bits, and nothing past dim written
    for x, y in zip(out_a, out_s):
        assert _same_bits(x, y)
    assert _same_bits(dq_a[:, :dim], dq_s[:, :dim])
    assert (dq_a[:, dim:] == 777.0).all() and (dq_s[:, dim:] == 777.0).all()
    lse_w, rl_w, wloss = (t.cpu().numpy() for t in out_a)
    got_dq = dq_a[:, :dim].cpu().numpy()
    # wloss and dq: one IEEE multiply each, bit for bit the restatement's
    ref_lw, ref_rw, ref_wl = weight_ref.fold(w, lse, rl)
    assert np.array_equal(wloss.view(np.int32), ref_wl.view(np.int32))
    ref_dq = weight_ref.scale_rows(w, before.cpu().numpy())
    assert np.array_equal(got_dq.view(np.int32), ref_dq.view(np.int32))
    one, zr, mid = w == 1, w == 0, (w > 0) & (w < 1)
    # weight 1: copies, dq untouched
    assert np.array_equal(lse_w[one].view(np.int32), lse[one].view(np.int32))
    assert np.array_equal(rl_w[one].view(np.int32), rl[one].view(np.int32))
    assert np.array_equal(wloss[one].view(np.int32), rl[one].view(np.int32))
    assert np.array_equal(got_dq[one].view(np.int32), vals.cpu().numpy()[one].view(np.int32))
    # weight 0: exactly (+0, +inf, +0, zeros)
    assert (wloss[zr].view(np.int32) == 0).all() and (rl_w[zr].view(np.int32) == 0).all()
    assert (lse_w[zr] == np.inf).all() and (got_dq[zr].view(np.int32) == 0).all()
    # in between: the formulas (libm within a few units; the tight bounds are in the libm test)
    assert np.allclose(lse_w[mid], ref_lw[mid], rtol=1e-6, atol=1e-6)
    assert np.allclose(rl_w[mid], ref_rw[mid], rtol=1e-5, atol=0)
    # outputs may alias the inputs; wloss and dq may be absent
    al, ar = tl.clone(), tr.clone()
    _native.check(_native.lib().tt_inbatch_weight_rows(tw.data_ptr(), al.data_ptr(), ar.data_ptr(), n, al.data_ptr(),
                                                       ar.data_ptr(), None, None, 0, 0,
                                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _same_bits(al, out_a[0]) and _same_bits(ar, out_a[1])


def test_invalid_weights_show_as_nan_in_their_rows_only(cuda):
    rng = np.random.default_rng(3)
    n, dim = 70, 20
    w = _weights(n, rng)
    lse = rng.uniform(-5, 12, n).astype(np.float32)
    rl = rng.uniform(0.01, 9, n).astype(np.float32)
    dq = torch.as_tensor(rng.standard_normal((n, dim)).astype(np.float32), device=cuda)
    tl, tr = torch.as_tensor(lse, device=cuda), torch.as_tensor(rl, device=cuda)
    d0 = dq.clone()
    good = [t.clone() for t in hip_ops.inbatch_weight_rows(torch.as_tensor(w, device=cuda), tl, tr, d0)]
    bad_rows = [3, 16, 69]
    wb = w.copy()
    wb[bad_rows] = [-1.0, 1.5, np.nan]
    d1 = dq.clone()
    got = [t.clone() for t in hip_ops.inbatch_weight_rows(torch.as_tensor(wb, device=cuda), tl, tr, d1)]
    torch.cuda.synchronize()
    keep = torch.ones(n, dtype=torch.bool, device=cuda)
    keep[bad_rows] = False
    for g, x in zip(got + [d1], good + [d0]):
        assert torch.isnan(g[~keep]).all()
        assert _same_bits(g[keep], x[keep])


def test_empty_batch_is_accepted(cuda):
    e = torch.empty(0, dtype=torch.float32, device=cuda)
    out = hip_ops.inbatch_weight_rows(e, e, e, torch.empty(0, 8, dtype=torch.float32, device=cuda))
    assert all(t.numel() == 0 for t in out)
    assert all(t.numel() == 0 for t in hip_ops.inbatch_weight_rows(e, e, e))


def test_wrapper_checks_its_arguments(cuda):
    x = torch.ones(4, device=cuda)
    with pytest.raises(ValueError, match="GPU"):
        hip_ops.inbatch_weight_rows(torch.ones(4), x, x)
    with pytest.raises(TypeError, match="float32"):
        hip_ops.inbatch_weight_rows(x.double(), x, x)
    with pytest.raises(ValueError, match="lse"):
        hip_ops.inbatch_weight_rows(x, torch.ones(5, device=cuda), x)
    with pytest.raises(ValueError, match="one row per weight"):
        hip_ops.inbatch_weight_rows(x, x, x, torch.ones(5, 8, device=cuda))


def test_libm_outputs_against_fp64(cuda):
    """lse_w: |lse_w - (lse - ln w)| <= 4 * 2^-23 * (|lse| + |ln w|) (one logf,
    one subtraction).  row_loss_w: -expm1(-row_loss_w), taken from the fp32
    output in fp64, within 8 * 2^-23 relative of w * (-expm1(-row_loss)) — the
    quantity the cols pass consumes (three libm calls and one multiply).
    Measured on the MI355X: see DESIGN (sample weights)."""
    rng = np.random.default_rng(11)
    n = 1 << 16
    w = np.exp(rng.uniform(np.log(1e-30), 0.0, n)).astype(np.float32)
    w = w[(w > 0) & (w < 1)]
    w = np.concatenate([w, np.float32([0.0, 1.0, 1e-30, np.nextafter(np.float32(1), np.float32(0))])])
    n = w.size
    rl = np.exp(rng.uniform(np.log(1e-7), np.log(90.0), n)).astype(np.float32)
    lse = rng.uniform(-60, 120, n).astype(np.float32)
    lse_w, rl_w, _ = (t.cpu().numpy() for t in hip_ops.inbatch_weight_rows(
        *(torch.as_tensor(x, device=cuda) for x in (w, lse, rl))))
    mid = (w > 0) & (w < 1)
    w64, l64, r64 = w[mid].astype(np.float64), lse[mid].astype(np.float64), rl[mid].astype(np.float64)
    e1 = np.abs(lse_w[mid].astype(np.float64) - (l64 - np.log(w64))) / (U * (np.abs(l64) + np.abs(np.log(w64))))
    want = w64 * -np.expm1(-r64)
    e2 = np.abs(-np.expm1(-rl_w[mid].astype(np.float64)) - want) / (U * want)
    print(f"lse_w: max {e1.max():.3f} units of 2^-23 (|lse| + |ln w|); "
          f"row_loss_w: max {e2.max():.3f} units of 2^-23 relative")
    assert np.isfinite(rl_w[mid]).all() and (rl_w[mid] > 0).all()
    assert e1.max() <= 4.0
    assert e2.max() <= 8.0
    assert lse_w[w == 0] == np.inf and rl_w[w == 0] == 0 and rl_w[w == 1] == rl[w == 1]


# ---- loss level ------------------------------------------------------------------------------
def _loss_problem(cuda, B, E, seed, duplicates=False):
    rng = np.random.default_rng(seed)
    q = np.maximum(rng.standard_normal((B, E)), 0).astype(np.float32)  # tower outputs are ReLU outputs
    c = np.maximum(rng.standard_normal((B, E)), 0).astype(np.float32)
    logq = np.log(rng.dirichlet(np.ones(max(B, 2)))[:B]).astype(np.float32)
    w = rng.uniform(0.0, 1.0, B).astype(np.float32)
    w[1::7] = 0.0
    w[3::7] = 1.0
    ids = None
    if duplicates:
        ids = rng.integers(1, 10 * B, B).astype(np.int32)
        ids[B // 2:] = ids[:B - B // 2]  # every candidate twice
        ids[5:9] = ids[4]
        ids[20:23] = 0  # out-of-vocabulary rows count as one candidate
    return q, c, logq, w, ids


def _rel(x, ref):
    """max |x - ref| relative to max |ref|; against an exactly zero reference
    (B = 1) the absolute value, the convention of tests/test_inbatch_hits_gpu.py."""
    x = x.detach().double().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)
    m = np.abs(ref).max()
    return float(np.abs(x - ref).max() / (m if m > 0 else 1.0))


def _weighted_loss_and_grads(cuda, q, c, logq, w, ids, scale):
    tq = torch.as_tensor(q, device=cuda).requires_grad_(True)
    tc = torch.as_tensor(c, device=cuda).requires_grad_(True)
    loss = losses.inbatch_softmax_xent(tq, tc, torch.as_tensor(logq, device=cuda),
                                       ids=None if ids is None else torch.as_tensor(ids, device=cuda),
                                       weights=torch.as_tensor(w, device=cuda), weight_scale=scale)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), tq.grad, tc.grad


def _check_x3(cuda, monkeypatch, B, E, duplicates):
    monkeypatch.setenv("TT_INBATCH_X3", "1")
    q, c, logq, w, ids = _loss_problem(cuda, B, E, 7 * B + E, duplicates)
    scale = 2.5
    ref = weight_ref.weighted_ref(q, c, logq, w.astype(np.float64) * scale, ids)
    loss, dq, dc = _weighted_loss_and_grads(cuda, q, c, logq, w, ids, scale)
    e_loss = abs(loss - ref["loss"]) / (abs(ref["loss"]) if ref["loss"] != 0 else 1.0)
    e_dq, e_dc = _rel(dq, ref["dq"]), _rel(dc, ref["dc"])
    print(f"x3 B={B} E={E} hits={duplicates}: loss {e_loss:.3g}, dQ {e_dq:.3g}, dC {e_dc:.3g}")
    assert e_dq <= 1e-3 and e_dc <= 1e-3
    assert e_loss <= 1e-4


def _check_bf16(cuda, B, E, duplicates):
    """Default arithmetic: the weighted error against fp64 is at most twice the
    unweighted rows -> cols chain's own error on the same q, c, logq, plus
    1e-6 (bf16(w p) rounds differently from bf16(p)).  The loss is compared
    term by term (max over rows, relative to the largest term): the sum's
    error depends on how the terms' errors cancel, the terms' do not."""
    q, c, logq, w, ids = _loss_problem(cuda, B, E, 7 * B + E, duplicates)
    tq, tc, tl, tw = (torch.as_tensor(x, device=cuda) for x in (q, c, logq, w))
    ti = None if ids is None else torch.as_tensor(ids, device=cuda)
    plain = weight_ref.weighted_ref(q, c, logq, None, ids)
    ref = weight_ref.weighted_ref(q, c, logq, w.astype(np.float64), ids)
    lse, rl, dq_u = hip_ops.inbatch_rows(tq, tc, tl, row_ids=ti, col_ids=ti)
    dc_u = hip_ops.inbatch_cols(tq, lse, tc, tl, row_loss=rl, row_ids=ti, col_ids=ti)
    u = (_rel(rl, plain["row_loss"]), _rel(dq_u, plain["dq"]), _rel(dc_u, plain["dc"]))
    wloss, dq, dc = losses.weighted_inbatch_grads(tq, tc, tl, tw, ti)
    wv = (_rel(wloss, w.astype(np.float64) * plain["row_loss"]), _rel(dq, ref["dq"]), _rel(dc, ref["dc"]))
    loss, gq, gc = _weighted_loss_and_grads(cuda, q, c, logq, w, ids, 1.0)
    assert torch.equal(gq, dq) and torch.equal(gc, dc)  # the public loss runs that chain
    assert loss == float(hip_ops.loss_sum(wloss.contiguous()))
    # the sum: sum_i w_i (rl_i - l_i) exactly, so within the weighted sum of the unweighted terms'
    # errors, plus the rounding of B products and B - 1 fp32 additions in any order
    term_err = np.abs(rl.double().cpu().numpy() - plain["row_loss"])
    assert abs(loss - ref["loss"]) <= float((w * term_err).sum()) + (B + 1) * 2.0 ** -24 * abs(ref["loss"])
    for name, a, b in zip(("loss terms", "dQ", "dC"), wv, u):
        print(f"bf16 B={B} E={E} hits={duplicates} {name}: weighted {a:.3g}, unweighted {b:.3g}")
    for name, a, b in zip(("loss terms", "dQ", "dC"), wv, u):
        assert a <= 2 * b + 1e-6, (name, a, b)


@pytest.mark.parametrize("E", [32, 100])
@pytest.mark.parametrize("B", [1, 33, 64, 200])
def test_weighted_loss_x3_against_fp64(cuda, monkeypatch, B, E):
    _check_x3(cuda, monkeypatch, B, E, False)


@pytest.mark.parametrize("E", [32, 100])
@pytest.mark.parametrize("B", [1, 33, 64, 200])
def test_weighted_loss_bf16_no_worse_than_unweighted(cuda, B, E):
    _check_bf16(cuda, B, E, False)


@pytest.mark.parametrize("mode", ["bf16", "x3"])
def test_weighted_loss_with_accidental_hits(cuda, monkeypatch, mode):
    if mode == "x3":
        _check_x3(cuda, monkeypatch, 200, 32, True)
    else:
        _check_bf16(cuda, 200, 32, True)


@pytest.mark.parametrize("reduction", ["sum", "mean", "sum_over_batch_size"])
def test_reductions_divide_by_the_batch_size(cuda, reduction):
    q, c, logq, w, _ = _loss_problem(cuda, 33, 32, 5)
    tq, tc, tl, tw = (torch.as_tensor(x, device=cuda) for x in (q, c, logq, w))
    got = losses.InBatchSoftmaxCrossEntropy(reduction=reduction)(tq, tc, tl, weights=tw, weight_scale=3.0)
    lse, rl, _ = hip_ops.inbatch_rows(tq, tc, tl, want_dq=False)
    _, _, wloss = hip_ops.inbatch_weight_rows(tw, lse, rl)
    scale = 1.0 if reduction == "sum" else 1.0 / 33
    assert torch.equal(got, hip_ops.loss_sum(wloss, scale * 3.0))  # Keras: sum(w l) / B, not / sum(w)


# ---- structure -------------------------------------------------------------------------------
@pytest.mark.parametrize("x3", [False, True])
def test_all_ones_is_the_unweighted_chain(cuda, x3):
    q, c, logq, _, _ = _loss_problem(cuda, 200, 100, 9)
    tq, tc, tl = (torch.as_tensor(x, device=cuda) for x in (q, c, logq))
    lse, rl, dq = hip_ops.inbatch_rows(tq, tc, tl, x3=x3)
    dc = hip_ops.inbatch_cols(tq, lse, tc, tl, row_loss=rl, x3=x3)
    lse2, rl2, dq2 = hip_ops.inbatch_rows(tq, tc, tl, x3=x3)
    lse_w, rl_w, wloss = hip_ops.inbatch_weight_rows(torch.ones(200, device=cuda), lse2, rl2, dq2)
    dc2 = hip_ops.inbatch_cols(tq, lse_w, tc, tl, row_loss=rl_w, x3=x3)
    for a, b in ((lse_w, lse), (rl_w, rl), (wloss, rl), (dq2, dq), (dc2, dc)):
        assert _same_bits(a, b)
    assert torch.equal(hip_ops.loss_sum(wloss.contiguous()), hip_ops.loss_sum(rl))


@pytest.mark.parametrize("x3", [False, True])
def test_weight_zero_rows_contribute_exactly_nothing(cuda, x3):
    B, E = 200, 32
    q, c, logq, w, _ = _loss_problem(cuda, B, E, 13)
    Z = w == 0
    assert 10 < Z.sum() < B // 2
    q2 = q.copy()
    q2[Z] = np.random.default_rng(1).uniform(0, 30, (int(Z.sum()), E)).astype(np.float32)
    tc, tl, tw = (torch.as_tensor(x, device=cuda) for x in (c, logq, w))
    runs = []
    for qq in (q, q2):
        wloss, dq, dc = losses.weighted_inbatch_grads(torch.as_tensor(qq, device=cuda), tc, tl, tw, x3=x3)
        runs.append((hip_ops.loss_sum(wloss.contiguous()).clone(), dq.clone(), dc.clone()))
    (la, dqa, dca), (lb, dqb, dcb) = runs
    tz = torch.as_tensor(Z, device=cuda)
    assert _same_bits(dca, dcb) and _same_bits(la, lb)
    assert _same_bits(dqa[~tz], dqb[~tz])
    assert (_bits(dqa[tz]) == 0).all() and (_bits(dqb[tz]) == 0).all()
    assert dca.abs().max() > 0


def _spy(monkeypatch, calls):
    for name in ("inbatch_fused", "inbatch_rows", "inbatch_cols", "inbatch_weight_rows", "loss_sum"):
        real = getattr(hip_ops, name)

        def wrapped(*a, _real=real, _name=name, **k):
            calls.append(_name)
            return _real(*a, **k)

        monkeypatch.setattr(hip_ops, name, wrapped)


def test_weights_none_issues_the_calls_it_issued_before(cuda, monkeypatch):
    calls = []
    _spy(monkeypatch, calls)
    q, c, logq, w, _ = _loss_problem(cuda, 64, 32, 2)
    tl, tw = torch.as_tensor(logq, device=cuda), torch.as_tensor(w, device=cuda)
    leaf = lambda x: torch.as_tensor(x, device=cuda).requires_grad_(True)
    m = _model(cuda, 0)
    x = _batch(cuda, np.random.default_rng(0), 64)
    # without weights: the fused entry (and tt_sum only where it always ran)
    losses.inbatch_softmax_xent(leaf(q), leaf(c), tl).backward()
    assert calls == ["inbatch_fused", "loss_sum"]
    del calls[:]
    losses.inbatch_softmax_xent(torch.as_tensor(q, device=cuda), torch.as_tensor(c, device=cuda), tl)
    assert calls == ["inbatch_rows", "loss_sum"]
    del calls[:]
    m.train_step(x)
    assert calls == ["inbatch_fused"]
    del calls[:]
    m.compute_loss(x, training=False)
    assert calls == ["inbatch_rows", "loss_sum"]
    del calls[:]
    # with weights: rows, fold, cols, tt_sum; no-grad evaluation: rows, fold, tt_sum
    losses.inbatch_softmax_xent(leaf(q), leaf(c), tl, weights=tw).backward()
    assert calls == ["inbatch_rows", "inbatch_weight_rows", "inbatch_cols", "loss_sum"]
    del calls[:]
    m.train_step(dict(x, **{WEIGHT_KEY: tw}))
    assert calls == ["inbatch_rows", "inbatch_weight_rows", "inbatch_cols", "loss_sum"]
    del calls[:]
    m.compute_loss(dict(x, **{WEIGHT_KEY: tw}), training=False)
    assert calls == ["inbatch_rows", "inbatch_weight_rows", "loss_sum"]


# ---- model level -----------------------------------------------------------------------------
B, E, H = 64, 32, 48
SCALE = 2.5


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
    m.sample_weight_scale = SCALE
    return m


def _batch(cuda, rng, n, weights=False):
    z = lambda v: torch.as_tensor(rng.integers(0, v, n).astype(np.int32), device=cuda)
    x = {"cust": z(301), "post": z(51), "art": z(301), "ptn": z(21)}
    if weights:
        w = rng.uniform(0.0, 1.0, n).astype(np.float32)
        w[1::6] = 0.0
        w[2::6] = 1.0
        x[WEIGHT_KEY] = torch.as_tensor(w, device=cuda)
    return x


def _state(m):
    out = {}
    for t, name in ((m.query_tower, "q"), (m.candidate_tower, "c")):
        out[name + ".mlp"] = t.dense.flat.detach().clone()
        out[name + ".mlp_acc"] = m.optimizer._slot(t.dense.flat, 1, 0.1)[0].clone()
        for n, layer in t.input_layer.embedding_layers.items():
            out[f"{name}.{n}"] = layer.weight.detach().clone()
            out[f"{name}.{n}.acc"] = m.optimizer._slot(layer.weight, 1, 0.1)[0].clone()
    return out


def _fp64_updates(m, x):
    """The Adagrad update of every parameter for the weighted loss of batch x,
    by torch fp64 autograd on a restatement of the model: embedding lookups,
    one hidden ReLU layer and a ReLU output layer per tower, S' = q.c^T -
    logq, L = scale * sum_i w_i (lse_i - S'_ii)."""
    opt = m.optimizer
    lr, eps, acc0 = opt.learning_rate, opt.epsilon, opt.initial_accumulator_value
    step = lambda g: -lr * g / (torch.sqrt(acc0 + g * g) + eps)
    outs, leaves = [], []
    for t in m.towers:
        layer = t.input_layer
        tabs = {f.name: layer.embedding_layers[f.name].weight.detach().double().requires_grad_(True)
                for f in layer.categorical_features}
        h = torch.cat([tabs[f.name][x[f.name].long()] for f in layer.categorical_features], 1)
        params = [(w.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True))
                  for w, b in t.dense.params()]
        for w, b in params:
            h = torch.relu(h @ w + b)
        outs.append(h)
        leaves.append((tabs, params))
    s = outs[0] @ outs[1].t() - m.candidate_logq(x).double()[None, :]
    loss = m.sample_weight_scale * (x[WEIGHT_KEY].double() * (torch.logsumexp(s, 1) - s.diagonal())).sum()
    loss.backward()
    upd = {}
    for name, (tabs, params) in zip("qc", leaves):
        for n, tab in tabs.items():
            touched = tab.grad.abs().sum(1, keepdim=True) > 0
            upd[f"{name}.{n}"] = torch.where(touched, step(tab.grad), torch.zeros_like(tab.grad))
        flat = torch.cat([torch.cat([w.grad.reshape(-1), b.grad]) for w, b in params])
        upd[f"{name}.mlp"] = step(flat)
    return float(loss.detach()), upd


def test_eager_weighted_step_against_fp64_restatement(cuda):
    """First-step parameter updates within the unweighted train-step tests'
    bounds of the fp64 restatement (tests/test_model_gpu.py: 3e-3 for the
    embedding tables, 1e-2 for the MLP buffers, relative in norm; loss 1e-3)."""
    m = _model(cuda, 4)
    x = _batch(cuda, np.random.default_rng(6), B, weights=True)
    ref_loss, upd = _fp64_updates(m, x)
    before = _state(m)
    loss = float(m.train_step(x)["loss"])
    after = _state(m)
    assert abs(loss - ref_loss) <= 1e-3 * abs(ref_loss)
    for k, d_ref in upd.items():
        d = (after[k] - before[k]).double()
        err = float((d - d_ref).norm() / d_ref.norm())
        print(f"weighted first-step update {k}: rel err {err:.2e}")
        assert err <= (1e-2 if k.endswith("mlp") else 3e-3), (k, err)
    # and it is not the unweighted step
    u = _model(cuda, 4)
    u.train_step({k: v for k, v in x.items() if k != WEIGHT_KEY})
    assert not torch.equal(_state(u)["c.art"], after["c.art"])


@pytest.mark.parametrize("path", ["dense_after_join", "fused_optimizer_apply", "graphed", "device_fit"])
def test_other_step_forms_train_bit_identically(cuda, monkeypatch, path):
    """Three weighted steps: every form of the step leaves the state of the
    default eager step (dense-early), bit for bit, and returns its losses."""
    rng = np.random.default_rng(8)
    batches = [_batch(cuda, rng, B, weights=True) for _ in range(3)]
    a = _model(cuda, 5)
    want = [a.train_step(x)["loss"].clone() for x in batches]
    b = _model(cuda, 5, fused_optimizer_apply=path == "fused_optimizer_apply")
    if path == "dense_after_join":
        monkeypatch.setattr(two_tower_model, "DENSE_EARLY", False)
    if path == "graphed":
        g = GraphedTrainStep(b, batches[0], warmup=1)
        assert g.weight_scale == SCALE and WEIGHT_KEY in g.float_keys
        got = [g.warmup_out["loss"].clone()] + [g(x)["loss"].clone() for x in batches[1:]]
    elif path == "device_fit":
        cols = {k: np.concatenate([x[k].cpu().numpy() for x in batches]) for k in batches[0]}
        ds = DeviceDataset.from_encoded(EncodedDataset(cols, batch_size=B, device=cuda, weight_scale=SCALE))
        assert ds.weight_scale == SCALE and ds.map(lambda t: t).weight_scale == SCALE
        b.sample_weight_scale = 1.0  # fit takes the scale from the dataset
        hist = b.fit(ds, epochs=1, use_graph=True)
        assert b.sample_weight_scale == SCALE and b._device_fit_graph.weight_scale == SCALE
        assert b._device_fit_graph.reusable(b, ds)
        mean = float(sum(w.double() for w in want).item()) / 3
        assert hist["loss"][0] == mean
        got = want
    else:
        got = [b.train_step(x)["loss"].clone() for x in batches]
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), (path, i)
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (path, k)
    a.optimizer.check_status(cuda)
    b.optimizer.check_status(cuda)


def test_evaluation_loss_equals_the_training_loss(cuda):
    for kw in ({}, {"remove_accidental_hits": True}):
        m = _model(cuda, 6, **kw)
        x = _batch(cuda, np.random.default_rng(3), B, weights=True)
        x["art"][B // 2:] = x["art"][:B // 2]
        ev = m.compute_loss(x, training=False).clone()
        tr = m.train_step(x)["loss"]
        assert torch.equal(ev, tr) and float(ev) > 0
        plain = {k: v for k, v in x.items() if k != WEIGHT_KEY}
        assert not torch.equal(_model(cuda, 6, **kw).compute_loss(plain, training=False), ev)


def test_graphed_step_keeps_to_what_it_was_captured_with(cuda):
    rng = np.random.default_rng(4)
    m = _model(cuda, 7)
    xw, xp = _batch(cuda, rng, B, weights=True), _batch(cuda, rng, B)
    g = GraphedTrainStep(m, xw, warmup=1)
    with pytest.raises(ValueError, match=WEIGHT_KEY):
        g(xp)
    with pytest.raises(ValueError, match=WEIGHT_KEY):
        g.pack(xp)
    assert g.reusable(m) and g.reusable(m, batch=xw) and not g.reusable(m, batch=xp)
    m.sample_weight_scale = 2 * SCALE  # the scale is a constant of the captured graph
    assert not g.reusable(m)
    m.sample_weight_scale = SCALE
    assert g.reusable(m)
    m2 = _model(cuda, 7)
    g2 = GraphedTrainStep(m2, xp, warmup=1)
    assert g2.weight_scale is None and g2.reusable(m2, batch=xp) and not g2.reusable(m2, batch=xw)
    with pytest.raises(ValueError, match=WEIGHT_KEY):
        g2(xw)


class _OneRank:
    """comm of a one-rank group (BatchComm without a process group)."""
    world, rank = 1, 0

    def all_gather(self, t):
        return t


@pytest.mark.parametrize("hits", [False, True])
def test_world1_global_loss_equals_the_single_device_loss(cuda, hits):
    m = _model(cuda, 9, remove_accidental_hits=hits)
    x = _batch(cuda, np.random.default_rng(5), B, weights=True)
    x["art"][B // 2:] = x["art"][:B // 2]
    q, c = m._split(x)
    with torch.no_grad():
        qi0, ci0 = m.query_tower.input_layer(q).clone(), m.candidate_tower.input_layer(c).clone()
    logq, ids, w = m.candidate_logq(x), m.candidate_ids(x), x[WEIGHT_KEY]
    assert (ids is not None) == hits
    sq, sc = m.query_tower.dense, m.candidate_tower.dense
    res = []
    for fn in (lambda qi, ci: losses.towers_inbatch_softmax_xent(qi, ci, sq, sc, logq, ids=ids, weights=w,
                                                                 weight_scale=SCALE),
               lambda qi, ci: losses.global_towers_inbatch_softmax_xent(qi, ci, sq, sc, _OneRank(), logq, ids=ids,
                                                                        weights=w, weight_scale=SCALE)):
        qi, ci = qi0.clone().requires_grad_(True), ci0.clone().requires_grad_(True)
        sq.flat.grad = sc.flat.grad = None
        loss = fn(qi, ci)
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach().clone(), sq.flat.grad.clone(), sc.flat.grad.clone(), qi.grad.clone(),
                    ci.grad.clone()))
    sq.flat.grad = sc.flat.grad = None
    assert float(res[0][0]) > 0 and res[0][1].abs().max() > 0
    for name, a, b in zip(("loss", "d flat_q", "d flat_c", "d qi", "d ci"), *res):
        assert torch.equal(a, b), name
