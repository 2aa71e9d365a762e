"""Hard-negative mining in the in-batch loss (num_hard_negatives; include/tt.h
"hard negatives") on the GPU: the selection kernel's thresholds and the HARD
form of the pass kernel through tt_inbatch_hard_threshold,
tt_inbatch_xent_rows_hard / _cols_hard and tt_inbatch_softmax_xent_hard, bf16
and x3, with and without candidate ids, against tests/hard_neg_ref.py.

Shapes (plan() of tests/inbatch_rowwise.py): n = 128 one workgroup and one
split; n = 200 padded rows and columns; rows 128 x cols 448 at pos_offset 192
(rows 192..319 of a batch of 448) rectangular, several splits of one tile;
n = 2112 16 planned splits of 3 tiles, some empty.
"""
import numpy as np
import pytest
import torch

import hard_neg_ref as hn
import inbatch_rowwise
from pkg.modelling import hip_ops

pytestmark = pytest.mark.gpu

# (n, (r0, r1)): the global batch and the rows / columns [r0, r1) of the "rank" under test
SHAPES = {"n128": (128, (0, 128)), "n200": (200, (0, 200)), "rect128x448": (448, (192, 320)),
          "n2112": (2112, (0, 2112))}
DIMS = (32, 64, 128)
FORMS = ("bf16", "x3")


def ks_of(negs):
    return sorted({1, 2, 63, 64, 65, negs - 1, negs, negs + 5})


def _ids(x, sl=None):
    if x["row_ids"] is None:
        return {}
    if sl is None:
        return {"row_ids": x["col_ids"], "col_ids": x["col_ids"]}
    return {"row_ids": x["col_ids"][sl], "col_ids": x["col_ids"]}


def _run(x, k, x3, r0, r1, fused):
    """thr and the loss of rows [r0, r1) / columns [r0, r1) of the batch:
    dict(thr_all, thr, lse, row_loss, dq (rows r0..r1), dc (columns r0..r1),
    fused (the single-device entry's outputs or None))."""
    q, c, logq = x["q"], x["c"], x["logq"]
    n = q.shape[0]
    sl = slice(r0, r1)
    ids_all = _ids(x)
    thr_all = hip_ops.inbatch_hard_threshold(q, c, logq, k, x3=x3, **ids_all)
    lse_all, loss_all, dq_all = hip_ops.inbatch_rows(q, c, logq, x3=x3, thr=thr_all, **ids_all)
    if (r0, r1) == (0, n):
        thr, lse, row_loss, dq = thr_all, lse_all, loss_all, dq_all
    else:
        thr = hip_ops.inbatch_hard_threshold(q[sl], c, logq, k, pos_offset=r0, x3=x3, **_ids(x, sl))
        lse, row_loss, dq = hip_ops.inbatch_rows(q[sl], c, logq, pos_offset=r0, x3=x3, thr=thr, **_ids(x, sl))
    ck = {} if x["row_ids"] is None else {"row_ids": x["col_ids"], "col_ids": x["col_ids"][sl]}
    dc = hip_ops.inbatch_cols(q, lse_all, c[sl], logq[sl], pos_offset=r0, row_loss=loss_all, x3=x3, thr=thr_all, **ck)
    out = {"thr_all": thr_all, "thr": thr, "lse": lse, "row_loss": row_loss, "dq": dq, "dc": dc, "fused": None}
    if fused:
        out["fused"] = hip_ops.inbatch_fused(q, c, logq, x3=x3, ids=x["col_ids"], hard_k=k)
    return out


def _bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# --------------------------------------------------------------------------- 1. exact arithmetic
@pytest.mark.parametrize("hits", [False, True], ids=["noids", "ids"])
@pytest.mark.parametrize("E", DIMS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_exact_inputs_thr_bitwise_and_per_element(cuda, shape, E, hits):
    n, (r0, r1) = SHAPES[shape]
    x = hn.to_torch(hn.exact_case(n, n, E, 0, hits), cuda)
    q, c, logq = x["q"], x["c"], x["logq"]
    S = hn.scores(q, c, logq, "fp64")  # exact: the kernels' S' in both arithmetics
    assert torch.equal(S, hn.scores(q, c, logq, "bf16")) and torch.equal(S, hn.scores(q, c, logq, "x3"))
    bad = []
    for k in ks_of(n - 1):
        sel = hn.select(S, k, 0, x["row_ids"], x["col_ids"])
        ref = hn.reference(q, c, logq, sel["kept"])
        ties = int(((sel["kept"].sum(1) > k) & torch.isfinite(sel["thr"])).sum())
        for form in FORMS:
            tag = f"{shape} E={E} k={k} {form}{' ids' if hits else ''}"
            out = _run(x, k, form == "x3", r0, r1, fused=(r0, r1) == (0, n))
            if not _bits(out["thr_all"], sel["thr"]):
                d = (out["thr_all"] != sel["thr"]).nonzero().flatten()
                bad.append(f"{tag}: thr differs in {d.numel()} rows, first {int(d[0])}: "
                           f"{float(out['thr_all'][d[0]])!r} ref {float(sel['thr'][d[0]])!r}")
                continue
            assert _bits(out["thr"], sel["thr"][r0:r1]), tag
            bnd = inbatch_rowwise.to_numpy(hn.bounds(ref, q, c, form))
            assert bool(bnd["certified"].all()), (tag, float(bnd["alpha"].max()))
            refn = inbatch_rowwise.to_numpy(ref)
            cut = {"lse": refn["lse"][r0:r1], "row_loss": refn["row_loss"][r0:r1], "dq": refn["dq"][r0:r1],
                   "dc": refn["dc"][r0:r1]}
            bcut = {kk: (v[r0:r1] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v)
                    for kk, v in bnd.items()}
            bad += inbatch_rowwise.violations(out, cut, bcut, d=refn["d"][r0:r1], tag=tag)
            if out["fused"] is not None:
                f = out["fused"]
                assert _bits(f[4], sel["thr"]), tag
                bad += inbatch_rowwise.violations(dict(zip(("lse", "row_loss", "dq", "dc"), f[:4])), refn, bnd,
                                                  d=refn["d"], tag=tag + " fused")
        print(f"{shape} E={E} k={k}: {ties} rows keep more than k (ties)")
    assert not bad, "\n".join(bad)


# --------------------------------------------------------------------------- 2. bit-equality to the existing entries
@pytest.mark.parametrize("hits", [False, True], ids=["noids", "ids"])
@pytest.mark.parametrize("x3", [False, True], ids=["bf16", "x3"])
@pytest.mark.parametrize("shape,E", [("n128", 32), ("n200", 64), ("rect128x448", 128), ("n2112", 128)])
def test_all_kept_equals_existing_entries_bitwise(cuda, shape, E, x3, hits):
    n, (r0, r1) = SHAPES[shape]
    B, E0, scale = (n, E, 0.25)
    xc = inbatch_rowwise.case(B, E0, scale, True, hits)
    q, c, logq = (torch.as_tensor(xc[k], device=cuda) for k in ("q", "c", "logq"))
    ids = None if xc["ids"] is None else torch.as_tensor(xc["ids"], device=cuda)
    x = {"q": q, "c": c, "logq": logq, "row_ids": ids, "col_ids": ids}
    sl = slice(r0, r1)
    rk = {} if ids is None else {"row_ids": ids[sl], "col_ids": ids}
    ck = {} if ids is None else {"row_ids": ids, "col_ids": ids[sl]}
    lse0, loss0, dq0 = hip_ops.inbatch_rows(q[sl], c, logq, pos_offset=r0, x3=x3, **rk)
    lse_all, loss_all, _ = hip_ops.inbatch_rows(q, c, logq, x3=x3, **_ids(x))
    dc0 = hip_ops.inbatch_cols(q, lse_all, c[sl], logq[sl], pos_offset=r0, row_loss=loss_all, x3=x3, **ck)
    ninf = torch.full((n,), float("-inf"), device=cuda)
    for label, k in (("k = negs", n - 1), ("k = negs + 5", n + 4), ("thr = -inf", None)):
        if k is None:
            thr, thr_all = ninf[sl].contiguous(), ninf
        else:
            thr = hip_ops.inbatch_hard_threshold(q[sl], c, logq, k, pos_offset=r0, x3=x3, **rk)
            thr_all = hip_ops.inbatch_hard_threshold(q, c, logq, k, x3=x3, **_ids(x))
            assert bool((thr == float("-inf")).all()) and bool((thr_all == float("-inf")).all()), label
        lse, loss, dq = hip_ops.inbatch_rows(q[sl], c, logq, pos_offset=r0, x3=x3, thr=thr, **rk)
        dc = hip_ops.inbatch_cols(q, lse_all, c[sl], logq[sl], pos_offset=r0, row_loss=loss_all, x3=x3, thr=thr_all,
                                  **ck)
        for name, got, want in (("lse", lse, lse0), ("row_loss", loss, loss0), ("dq", dq, dq0), ("dc", dc, dc0)):
            assert _bits(got, want), (shape, label, name)
    if (r0, r1) == (0, n):
        base = hip_ops.inbatch_fused(q, c, logq, x3=x3, ids=ids, loss_scale=0.5)
        hard = hip_ops.inbatch_fused(q, c, logq, x3=x3, ids=ids, loss_scale=0.5, hard_k=n + 4)
        for i, name in enumerate(("lse", "row_loss", "dq", "dc")):
            assert _bits(hard[i], base[i]), (shape, "fused", name)
        assert _bits(hard[5].reshape(1), base[4].reshape(1)) and bool((hard[4] == float("-inf")).all())


# --------------------------------------------------------------------------- 3. rank validity on trained-regime inputs
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,E,scale", [(129, 37, 0.45), (65, 16, 0.6), (2080, 128, 0.25)])  # of inbatch_rowwise.TRAINED
def test_random_inputs_thr_has_rank_k(cuda, B, E, scale, form):
    for hits in (False, True):
        xc = inbatch_rowwise.case(B, E, scale, True, hits)
        q, c, logq = (torch.as_tensor(xc[k], device=cuda) for k in ("q", "c", "logq"))
        ids = None if xc["ids"] is None else torch.as_tensor(xc["ids"], device=cuda)
        kw = {} if ids is None else {"row_ids": ids, "col_ids": ids}
        Sref = hn.scores(q, c, logq, "fp64")
        delta = hn.score_delta(q, c, form)
        for k in ks_of(B - 1):
            thr = hip_ops.inbatch_hard_threshold(q, c, logq, k, x3=form == "x3", **kw)
            lo, hi = hn.rank_window(Sref, thr, delta, 0, ids, ids)
            fin = torch.isfinite(thr)
            # thr = -inf: the row has at most k finite negatives
            nfin = hn.rank_window(Sref, torch.full_like(thr, -3e38), delta, 0, ids, ids)[1]
            assert bool((nfin[~fin] <= k).all()), (B, form, hits, k)
            ok = (lo <= k) & (k <= hi)
            assert bool(ok[fin].all()), (B, form, hits, k, int((~ok & fin).sum()),
                                         int((~ok & fin).nonzero()[0]))
            if k >= B - 1:
                assert not bool(fin.any())


# --------------------------------------------------------------------------- 4. end to end with a certified gap
@pytest.mark.parametrize("form", FORMS)
def test_gap_case_end_to_end(cuda, form):
    x = hn.to_torch(hn.gap_case(), cuda)
    q, c, logq = x["q"], x["c"], x["logq"]
    k = hn.GAP_K
    sel = hn.select(hn.scores(q, c, logq, "fp64"), k)
    delta = hn.score_delta(q, c, form)
    assert bool(((sel["a"] - sel["b"]) > 64 * delta).all())
    ref = hn.reference(q, c, logq, sel["kept"])
    bnd = inbatch_rowwise.to_numpy(hn.bounds(ref, q, c, form))
    assert bool(bnd["certified"].all())
    refn = inbatch_rowwise.to_numpy(ref)
    x3 = form == "x3"
    thr = hip_ops.inbatch_hard_threshold(q, c, logq, k, x3=x3)
    assert bool(((thr.double() < sel["a"] - 31 * delta) & (thr.double() > sel["b"] + 31 * delta)).all())
    lse, row_loss, dq = hip_ops.inbatch_rows(q, c, logq, x3=x3, thr=thr)
    dc = hip_ops.inbatch_cols(q, lse, c, logq, row_loss=row_loss, x3=x3, thr=thr)
    bad = inbatch_rowwise.violations({"lse": lse, "row_loss": row_loss, "dq": dq, "dc": dc}, refn, bnd, d=refn["d"],
                                     tag=f"gap {form} rows+cols")
    f = hip_ops.inbatch_fused(q, c, logq, x3=x3, hard_k=k, loss_scale=1.0)
    bad += inbatch_rowwise.violations(dict(zip(("lse", "row_loss", "dq", "dc"), f[:4])), refn, bnd, d=refn["d"],
                                      tag=f"gap {form} fused")
    assert not bad, "\n".join(bad)
    assert _bits(f[4], thr)
    assert abs(float(f[5]) - refn["row_loss"].sum()) <= float(bnd["row_loss"].sum()) + 1e-5 * refn["row_loss"].sum()
    # mining matters here: the unmasked loss is far outside the bounds
    plain = hip_ops.inbatch_fused(q, c, logq, x3=x3)
    assert inbatch_rowwise.violations(dict(zip(("lse", "row_loss", "dq", "dc"), plain[:4])), refn, bnd, d=refn["d"])


# --------------------------------------------------------------------------- 5. composition with sample weights
@pytest.mark.parametrize("form", FORMS)
def test_weights_compose(cuda, form):
    from pkg.modelling import losses

    x = hn.to_torch(hn.gap_case(), cuda)
    q, c, logq = x["q"], x["c"], x["logq"]
    k, x3 = hn.GAP_K, form == "x3"
    sel = hn.select(hn.scores(q, c, logq, "fp64"), k)
    ref = hn.reference(q, c, logq, sel["kept"])
    w = torch.linspace(0.0, 1.0, q.shape[0], device=cuda)
    wloss, dq, dc = losses.weighted_inbatch_grads(q, c, logq, w, x3=x3, num_hard_negatives=k)
    want = float((w.double() * ref["row_loss"]).sum())
    tol = 1e-4 if x3 else 1e-3  # the weighted tests' loss tolerances (tests/test_weight_gpu.py)
    assert abs(float(wloss.double().sum()) - want) <= tol * abs(want), (float(wloss.sum()), want)
    # the gradients: those of the unweighted masked loss with rows scaled by w
    dq_ref = w.double()[:, None] * ref["dq"]
    assert float((dq.double() - dq_ref).norm() / dq_ref.norm()) <= 10 * tol
    assert bool((dq[0] == 0).all())
    # weights all one: the unweighted hard entries' values
    one = torch.ones_like(w)
    wl1, dq1, dc1 = losses.weighted_inbatch_grads(q, c, logq, one, x3=x3, num_hard_negatives=k)
    f = hip_ops.inbatch_fused(q, c, logq, x3=x3, hard_k=k)
    for got, want in ((dq1, f[2]), (dc1, f[3])):  # the same sums, possibly split otherwise: fp32 rounding
        assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())


# --------------------------------------------------------------------------- cross-pass agreement on exact ties
@pytest.mark.parametrize("form", FORMS)
def test_rows_and_cols_keep_the_same_pairs_at_exact_ties(cuda, form):
    """Duplicate candidates passed WITHOUT ids: columns i and i + 7 score the
    same in every row, so wherever they hold ranks k and k + 1 thr equals
    their score and the pair is kept only if the cols pass forms that score
    to the bit.  sum_i dq_i . q_i and sum_j dc_j . c_j are the same sum over
    the kept pairs (sum_ij P_ij S_ij less the positives' terms), each pass's
    own; their difference is bounded by the passes' rounding of p (2^-8 for
    bf16, 3 * 2^-17 for x3: oracle.BF16_P_U / X3_P_U, times 4 for the two
    operand roundings and the fp32 sums) on sum |dq . q| + |dc . c|, far
    below one dropped tie (~1e-2 of it when half the tied rows disagree)."""
    from oracle import oracle

    xc = inbatch_rowwise.case(2080, 128, 0.25, True, True)
    q, c, logq = (torch.as_tensor(xc[k], device=cuda) for k in ("q", "c", "logq"))
    S = hn.scores(q, c, logq, "fp64")
    u = oracle.X3_P_U if form == "x3" else oracle.BF16_P_U
    for k in (1, 2, 8, 64):
        sel = hn.select(S, k)
        tied = int((sel["a"] == sel["b"]).sum())
        assert tied > 0, k  # the input has such rows at every k used
        thr = hip_ops.inbatch_hard_threshold(q, c, logq, k, x3=form == "x3")
        lse, row_loss, dq = hip_ops.inbatch_rows(q, c, logq, x3=form == "x3", thr=thr)
        dc = hip_ops.inbatch_cols(q, lse, c, logq, row_loss=row_loss, x3=form == "x3", thr=thr)
        tq, tc = (dq.double() * q.double()).sum(1), (dc.double() * c.double()).sum(1)
        diff, size = abs(float(tq.sum() - tc.sum())), float(tq.abs().sum() + tc.abs().sum())
        print(f"{form} k={k}: {tied} tied rows, |sum dq.q - sum dc.c| = {diff:.3e} of {size:.3e} ({diff / size:.2e})")
        assert diff <= 4 * u * size, (form, k, diff, size)


# --------------------------------------------------------------------------- 5b / 6. the model
from pkg import dtypes  # noqa: E402
from pkg.modelling.dataset import DeviceDataset, EncodedDataset  # noqa: E402
from pkg.modelling.models.two_tower_model import GraphedTrainStep, TwoTowerModel  # noqa: E402
from pkg.modelling.optimizer_factory import OptimizerFactory  # noqa: E402
from pkg.schema.features import Feature, FeatureFamily  # noqa: E402

MB, ME, MH, MK = 128, 32, 48, 16


def _model(cuda, seed=0, **kw):
    V = [str(i) for i in range(300)]
    qf = [Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=16, vocab=V),
          Feature("post", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V[:50])]
    cf = [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=16, vocab=V),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=V[:20])]
    rng = np.random.default_rng(seed)
    probs = {str(i): float(p) for i, p in enumerate(rng.dirichlet(np.ones(300)))}
    m = TwoTowerModel(qf, cf, "art", ME, [MH], [MH], probs, device=cuda, seed=seed, **kw)
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", {"learning_rate": 0.05}))
    return m


def _batch(cuda, rng, n):
    z = lambda v: torch.as_tensor(rng.integers(0, v, n).astype(np.int32), device=cuda)  # noqa: E731
    return {"cust": z(301), "post": z(51), "art": z(301), "ptn": z(21)}


def _state(m):
    out = {}
    for t, name in ((m.query_tower, "q"), (m.candidate_tower, "c")):
        out[name + ".mlp"] = t.dense.flat.detach().clone()
        for n, layer in t.input_layer.embedding_layers.items():
            out[f"{name}.{n}"] = layer.weight.detach().clone()
    return out


def _fp64_loss(m, x, k):
    """The model's loss on batch x restated in torch fp64 (embedding lookups,
    the towers' ReLU layers, optional cosine / temperature, logQ, accidental
    hits, then the k hardest negatives of each row by a full sort)."""
    outs = []
    for t in m.towers:
        layer = t.input_layer
        h = torch.cat([layer.embedding_layers[f.name].weight.detach().double()[x[f.name].long()]
                       for f in layer.categorical_features], 1)
        for w, b in t.dense.params():
            h = torch.relu(h @ w.detach().double() + b.detach().double())
        if m.normalize_embeddings:
            h = h / h.norm(dim=1, keepdim=True).clamp_min(1e-30)
        outs.append(h)
    qo = outs[0] / (m.temperature or 1.0)
    logq = m.candidate_logq(x)
    ids = m.candidate_ids(x)
    sel = hn.select(hn.scores(qo, outs[1], logq, "fp64"), k, 0, ids, ids)
    ref = hn.reference(qo, outs[1], logq, sel["kept"])
    return ref["loss"]


def test_model_k_above_the_batch_is_the_default_step_bitwise(cuda):
    rng = np.random.default_rng(11)
    batches = [_batch(cuda, rng, MB) for _ in range(2)]
    a, b = _model(cuda, 3), _model(cuda, 3, num_hard_negatives=MB + 10)
    for x in batches:
        la, lb = a.train_step(x)["loss"], b.train_step(x)["loss"]
        assert torch.equal(la, lb)
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.compute_loss(batches[0], training=False), b.compute_loss(batches[0], training=False))


@pytest.mark.parametrize("kw", [{}, {"remove_accidental_hits": True},
                                {"normalize_embeddings": True, "temperature": 0.1}],
                         ids=["plain", "hits", "cosine"])
def test_model_loss_against_fp64(cuda, kw):
    """Training and evaluation loss of a model with num_hard_negatives = 16 at
    B = 128 within the model tests' loss tolerance (1e-3 relative,
    tests/test_weight_gpu.py / tests/test_model_gpu.py) of the fp64 restatement."""
    m = _model(cuda, 4, num_hard_negatives=MK, **kw)
    x = _batch(cuda, np.random.default_rng(6), MB)
    x["art"][MB // 2:MB // 2 + 16] = x["art"][:16]  # duplicate candidates
    want = _fp64_loss(m, x, MK)
    plain = _fp64_loss(m, x, MB + 10)
    assert abs(plain - want) > 0.01 * abs(want)  # mining changes this loss by far more than the tolerance
    ev = float(m.compute_loss(x, training=False))
    tr = float(m.train_step(x)["loss"])
    print(f"{kw}: loss {tr:.6f}, eval {ev:.6f}, fp64 {want:.6f} (unmined {plain:.6f})")
    assert ev == tr
    assert abs(tr - want) <= 1e-3 * abs(want)


@pytest.mark.parametrize("path", ["fused_optimizer_apply", "graphed", "device_fit"])
def test_model_step_forms_train_bit_identically(cuda, path):
    """Three steps with num_hard_negatives = 16: every form of the step leaves
    the eager step's state bit for bit and returns its losses."""
    rng = np.random.default_rng(8)
    batches = [_batch(cuda, rng, MB) for _ in range(3)]
    a = _model(cuda, 5, num_hard_negatives=MK)
    want = [a.train_step(x)["loss"].clone() for x in batches]
    d = _model(cuda, 5)
    assert not torch.equal(d.train_step(batches[0])["loss"], want[0])  # and it is not the default step
    b = _model(cuda, 5, num_hard_negatives=MK, fused_optimizer_apply=path == "fused_optimizer_apply")
    if path == "graphed":
        g = GraphedTrainStep(b, batches[0], warmup=1)
        got = [g.warmup_out["loss"].clone()] + [g(x)["loss"].clone() for x in batches[1:]]
    elif path == "device_fit":
        cols = {k: np.concatenate([x[k].cpu().numpy() for x in batches]) for k in batches[0]}
        ds = DeviceDataset.from_encoded(EncodedDataset(cols, batch_size=MB, device=cuda))
        hist = b.fit(ds, epochs=1, use_graph=True)
        assert hist["loss"][0] == float(sum(w.double() for w in want).item()) / 3
        got = want
    else:
        got = [b.train_step(x)["loss"].clone() for x in batches]
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), (path, i)
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (path, k)


def test_model_save_load_keeps_the_setting(cuda, tmp_path):
    m = _model(cuda, 2, num_hard_negatives=7)
    m.save(str(tmp_path / "m"))
    r = TwoTowerModel.load(str(tmp_path / "m"), device=cuda)
    assert r.num_hard_negatives == 7
    x = _batch(cuda, np.random.default_rng(1), MB)
    assert torch.equal(m.compute_loss(x, training=False), r.compute_loss(x, training=False))
    d = _model(cuda, 2)
    d.save(str(tmp_path / "d"))
    assert TwoTowerModel.load(str(tmp_path / "d"), device=cuda).num_hard_negatives is None


@pytest.mark.parametrize("k", [0, -1, 2.5])
def test_model_refuses_a_bad_k(cuda, k):
    with pytest.raises(ValueError, match="num_hard_negatives"):
        _model(cuda, 0, num_hard_negatives=k)


def test_world1_global_loss_equals_the_single_device_loss(cuda):
    """losses.global_inbatch_grads(num_hard_negatives=...) at one rank: the
    fused shortcut and the rows / gather / cols form give the fused entry's
    values (the same plan at n = 128: bit for bit)."""
    from pkg.modelling import losses

    class Comm:
        world, rank = 1, 0

        def all_gather(self, t):
            return t

    class Always(Comm):
        always = True

    x = hn.to_torch(hn.gap_case(), cuda)
    q, c, logq = x["q"], x["c"], x["logq"]
    f = hip_ops.inbatch_fused(q, c, logq, hard_k=hn.GAP_K)
    row_loss, dq, dc = losses.global_inbatch_grads(q, c, logq, Comm(), x3=False, num_hard_negatives=hn.GAP_K)
    assert _bits(row_loss, f[1]) and _bits(dq, f[2]) and _bits(dc, f[3])
    row_loss, dq, dc = losses.global_inbatch_grads(q, c, logq, Always(), x3=False, num_hard_negatives=hn.GAP_K)
    for got, want in ((row_loss, f[1]), (dq, f[2]), (dc, f[3])):  # the same sums: fp32 rounding at most
        assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())
