"""Mixed negative sampling on the GPU (include/tt.h, "mixed negatives"):
tt_mixed_candidates against the numpy sampler bit for bit, the MIXED column
pass and the fused q [n] x c [n + m] entry against the existing entries (bit
for bit where the arithmetic is the same), the bf16 contract and fp64, and
TwoTowerModel(num_sampled_negatives=M) on every form of the train step.

Shapes (n, m) are mixed_neg_ref.SHAPES: (100, 37) puts the extra columns'
would-be positives into the streamed padding, (64, 200) beyond the padded
streamed extent with several stationary blocks.
"""
import numpy as np
import pytest
import torch

import inbatch_rowwise as ir
import mixed_neg_ref as mn
from oracle import oracle
from pkg import dtypes
from pkg.modelling import hip_ops, losses
from pkg.modelling.dataset import CandidateCatalogue, DeviceDataset, EncodedDataset
from pkg.modelling.models.two_tower_model import GraphedTrainStep, TwoTowerModel
from pkg.modelling.optimizer_factory import OptimizerFactory
from pkg.schema.features import Feature, FeatureFamily

pytestmark = pytest.mark.gpu

FORMS = ("bf16", "x3")
NAMES = ("lse", "row_loss", "dq", "dc")


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _dev(x, cuda, logq=True):
    q, c = torch.as_tensor(x["q"], device=cuda), torch.as_tensor(x["c"], device=cuda)
    lq = torch.as_tensor(x["logq"], device=cuda) if logq else None
    ids = None if x["ids"] is None else torch.as_tensor(x["ids"], device=cuda)
    return q, c, lq, ids


# --------------------------------------------------------------------------- tt_mixed_candidates
@pytest.mark.parametrize("N", [1, 7, 105542])
@pytest.mark.parametrize("B", [5, 256])
def test_mixed_candidates_equals_the_restatement_bitwise(cuda, B, N):
    rng = np.random.default_rng(B + N)
    cat = np.stack([rng.integers(0, 1 << 30, N).astype(np.int32), rng.integers(0, 50, N).astype(np.int32),
                    rng.standard_normal(N).astype(np.float32).view(np.int32)])
    cols = [rng.integers(0, 1 << 30, B).astype(np.int32), rng.integers(0, 50, B).astype(np.int32),
            rng.standard_normal(B).astype(np.float32)]
    dcat = torch.as_tensor(cat, device=cuda)
    dcols = [torch.as_tensor(v, device=cuda) for v in cols]
    for M in (1, 3, 4, 1023):
        for seed, step0 in ((0, 0), (0x1234567800000009, (1 << 32) - 2)):  # the step's carry into its high word
            step = torch.full((1,), step0, dtype=torch.int64, device=cuda)
            status = torch.zeros(1, dtype=torch.int32, device=cuda)
            out = torch.full((3, B + M + 3), -7, dtype=torch.int32, device=cuda)  # dst_ld > B + M
            for launch in range(3):
                hip_ops.mixed_candidates(dcols, dcat, M, seed, step, out, status)
                want = mn.assemble(cols, cat, M, seed, step0 + launch)
                got = out.cpu().numpy()
                assert np.array_equal(got[:, :B + M], want), (B, M, N, seed, launch)
                assert (got[:, B + M:] == -7).all()
                assert int(step.item()) == step0 + launch + 1
            assert int(status.item()) == 0


def test_mixed_candidates_flags_an_unusable_catalogue_size(cuda):
    cat = torch.arange(8, dtype=torch.int32, device=cuda).view(1, 8)
    col = [torch.arange(4, dtype=torch.int32, device=cuda)]
    step = torch.zeros(1, dtype=torch.int64, device=cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    out = torch.full((1, 7), 5, dtype=torch.int32, device=cuda)
    hip_ops.mixed_candidates(col, cat, 3, 0, step, out, status, n_cat=0)
    assert out.cpu().tolist() == [[0, 1, 2, 3, 0, 0, 0]] and int(status.item()) == 1
    with pytest.raises(Exception, match="n_cat"):
        hip_ops.mixed_candidates(col, cat, 3, 0, step, out, None, n_cat=0)


# --------------------------------------------------------------------------- m = 0 and square: the existing entries
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("E", mn.DIMS)
def test_m0_equals_the_fused_entries_bitwise(cuda, E, form):
    x3 = form == "x3"
    for n, _ in mn.SHAPES:
        for logq_on in (True, False):
            q, c, lq, ids = _dev(mn.case(n, 0, E, hits=True), cuda, logq_on)
            for label, kw in (("plain", {}), ("hits", {"ids": ids}), ("hard", {"hard_k": 5}),
                              ("hits+hard", {"ids": ids, "hard_k": 5})):
                want = hip_ops.inbatch_fused(q, c, lq, loss_scale=0.5, x3=x3, **kw)
                got = hip_ops.inbatch_fused_mixed(q, c, lq, loss_scale=0.5, x3=x3, **kw)
                assert len(got) == len(want)
                for i, (a, b) in enumerate(zip(got, want)):
                    assert _bits(a.reshape(-1), b.reshape(-1)), (n, E, form, logq_on, label, i)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("E", mn.DIMS)
def test_cols_mixed_with_every_positive_present_equals_the_cols_entries_bitwise(cuda, E, form):
    x3 = form == "x3"
    for n, _ in mn.SHAPES:
        q, c, lq, ids = _dev(mn.case(n, 0, E, hits=True), cuda)
        for off, cs in ((0, slice(0, n)), (7, slice(7, n - 3))):  # n_cols + pos_offset <= n_rows
            for hits in (False, True):
                rk = {"row_ids": ids, "col_ids": ids} if hits else {}
                ck = {"row_ids": ids, "col_ids": ids[cs].contiguous()} if hits else {}
                for k in (None, 5):
                    thr = None if k is None else hip_ops.inbatch_hard_threshold(q, c, lq, k, x3=x3, **rk)
                    lse, row_loss, _ = hip_ops.inbatch_rows(q, c, lq, x3=x3, thr=thr, **rk)
                    cc, lc = c[cs].contiguous(), lq[cs].contiguous()
                    want = hip_ops.inbatch_cols(q, lse, cc, lc, pos_offset=off, row_loss=row_loss, x3=x3, thr=thr, **ck)
                    got = hip_ops.inbatch_cols(q, lse, cc, lc, pos_offset=off, row_loss=row_loss, x3=x3, thr=thr,
                                               mixed=True, **ck)
                    assert _bits(got, want), (n, E, form, off, hits, k)
                    nl = hip_ops.inbatch_cols(q, lse, cc, lc, pos_offset=off, x3=x3, thr=thr, mixed=True, **ck)
                    assert _bits(nl, hip_ops.inbatch_cols(q, lse, cc, lc, pos_offset=off, x3=x3, thr=thr, **ck))


# --------------------------------------------------------------------------- m > 0
def _check_dc(tag, dc, q, c, lq, lse, row_loss, n, form, rid=None, cid=None):
    """dc of a MIXED pass: the bf16 contract per element (columns < n against
    oracle.inbatch_cols_bf16, columns >= n against the same arithmetic without
    the positive's term), for the bf16 form."""
    if form != "bf16":
        return []
    qn, cn, lsen, lossn = (t.cpu().numpy() for t in (q, c, lse, row_loss))
    lqn = None if lq is None else lq.cpu().numpy()
    rn, cidn = (None, None) if rid is None else (rid.cpu().numpy(), cid.cpu().numpy())
    con, bnd = oracle.inbatch_cols_bf16(qn, lsen, lossn, cn[:n], None if lqn is None else lqn[:n], 0, 2048, rn,
                                        None if cidn is None else cidn[:n], True)
    con2, bnd2 = mn.cols_no_pos_bf16(qn, lsen, cn[n:], None if lqn is None else lqn[n:], rn,
                                     None if cidn is None else cidn[n:])
    return ir.violations({"dc": dc}, {"dc": np.concatenate([con, con2])}, {"dc": np.concatenate([bnd, bnd2])},
                         keys=("dc",), tag=tag + " dc vs contract")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("E", mn.DIMS)
@pytest.mark.parametrize("n,m", [s for s in mn.SHAPES])
def test_fused_mixed(cuda, n, m, E, form):
    """Rows side bit for bit the rows / threshold entries' at n_cols = n + m;
    dc per element against the bf16 contract and against fp64 (certified
    bounds of tests/inbatch_rowwise.py, every row certified; x3 also 1e-3 in
    norm and the loss 1e-4); reruns bit-identical; with and without logQ, ids
    and mining."""
    x3 = form == "x3"
    bad = []
    for logq_on in (True, False):
        for hits in (False, True):
            q, c, lq, ids = _dev(mn.case(n, m, E, hits=hits), cuda, logq_on)
            rid = None if ids is None else ids[:n]
            rk = {} if ids is None else {"row_ids": rid, "col_ids": ids}
            for k in (None, 7):
                tag = f"n={n} m={m} E={E} {form} logq={logq_on} hits={hits} k={k}"
                out = hip_ops.inbatch_fused_mixed(q, c, lq, loss_scale=0.5, x3=x3, ids=ids, hard_k=k)
                lse, row_loss, dq, dc = out[:4]
                assert tuple(dc.shape) == (n + m, E)
                thr = None
                if k is not None:
                    thr = hip_ops.inbatch_hard_threshold(q, c, lq, k, x3=x3, **rk)
                    assert _bits(out[4], thr), tag
                r = hip_ops.inbatch_rows(q, c, lq, x3=x3, thr=thr, **rk)
                for name, a, b in zip(NAMES, (lse, row_loss, dq), r):
                    assert _bits(a, b), (tag, name)
                assert _bits(out[-1].reshape(1), hip_ops.loss_sum(row_loss, 0.5).reshape(1)), tag
                # the MIXED cols entry on the same operands: the fused entry's dc
                dc2 = hip_ops.inbatch_cols(q, lse, c, lq, row_loss=row_loss, x3=x3, thr=thr, mixed=True, **rk)
                assert _bits(dc2, dc), tag
                again = hip_ops.inbatch_fused_mixed(q, c, lq, loss_scale=0.5, x3=x3, ids=ids, hard_k=k)
                for i, (a, b) in enumerate(zip(again, out)):
                    assert _bits(a.reshape(-1), b.reshape(-1)), (tag, "rerun", i)
                if k is not None:
                    continue  # mining: test_weights_and_mining_compose
                bad += _check_dc(tag, dc, q, c, lq, lse, row_loss, n, form, rid, ids)
                ref = ir.reference_torch(q, c, lq, 0, rid, ids)
                bnd = ir.to_numpy(ir.bounds_torch(ref, q, c, *ir.FORMS[form]))
                assert bool(bnd["certified"].all()), (tag, float(bnd["alpha"].max()))
                refn = ir.to_numpy(ref)
                bad += ir.violations(dict(zip(NAMES, out[:4])), refn, bnd, d=refn["d"], tag=tag + " vs fp64")
                if ids is None:  # ... and oracle.inbatch_softmax_xent (R < C, fp64)
                    o = oracle.inbatch_softmax_xent(q.cpu().numpy(), c.cpu().numpy(),
                                                    None if lq is None else lq.cpu().numpy())
                    for name, got in (("dq", dq), ("dc", dc)) if x3 else ():  # (bf16: the per-element bounds above)
                        err = np.linalg.norm(got.cpu().numpy() - o[name]) / np.linalg.norm(o[name])
                        assert err <= 1e-3, (tag, name, err)
                    assert abs(2.0 * float(out[-1]) - o["loss"]) <= (1e-4 if x3 else 1e-3) * abs(o["loss"]), tag
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("form", FORMS)
def test_hits_mask_sampled_columns(cuda, form):
    """ids with a sampled column (n) equal to row 3's positive id and one
    (n + 1) equal to nobody's: the pair (3, n) has weight 0 in lse, dq and dc
    — the outputs equal those of the problem with that ONE pair removed by
    hand (fp64) — and a column masked for every row gets dc = 0 exactly."""
    x3 = form == "x3"
    n, m, E = 100, 37, 48
    q, c, lq, ids = _dev(mn.case(n, m, E, hits=True), cuda)
    out = hip_ops.inbatch_fused_mixed(q, c, lq, x3=x3, ids=ids)
    plain = hip_ops.inbatch_fused_mixed(q, c, lq, x3=x3)
    # rows other than 3, 5 and 9 (pairs (3, n), (5, 9), (9, 5) are hits) are untouched by the ids
    keep = torch.ones(n, dtype=torch.bool, device=cuda)
    keep[[3, 5, 9]] = False
    assert _bits(out[0][keep], plain[0][keep]) and _bits(out[2][keep], plain[2][keep])
    assert not _bits(out[0][3:4], plain[0][3:4])
    # the fp64 reference by ids is the problem with exactly those three pairs removed by hand
    rt = ir.reference_torch(q, c, lq, 0, ids[:n], ids)
    ref = ir.to_numpy(rt)
    S = (q.double() @ c.double().T - lq.double()[None, :])
    S[3, n] = S[5, 9] = S[9, 5] = float("-inf")
    assert np.allclose(ref["lse"], torch.logsumexp(S, 1).cpu().numpy(), rtol=0, atol=1e-12)
    bnd = ir.to_numpy(ir.bounds_torch(rt, q, c, *ir.FORMS[form]))
    assert bool(bnd["certified"].all())
    bad = ir.violations(dict(zip(NAMES, out[:4])), ref, bnd, d=ref["d"], tag=f"hits {form}")
    assert not bad, "\n".join(bad)
    # a column masked for every row: every row carries id 7, and so does sampled column n + 2
    row_ids = torch.full((n,), 7, dtype=torch.int32, device=cuda)
    col_ids = torch.arange(100, 100 + n + m, dtype=torch.int32, device=cuda)
    col_ids[n + 2] = 7
    lse, row_loss, dq = hip_ops.inbatch_rows(q, c, lq, x3=x3, row_ids=row_ids, col_ids=col_ids)
    dc = hip_ops.inbatch_cols(q, lse, c, lq, row_loss=row_loss, x3=x3, row_ids=row_ids, col_ids=col_ids, mixed=True)
    assert bool((dc[n + 2] == 0).all()) and bool((dc[n + 1] != 0).any())
    w = hip_ops.inbatch_rows(q, torch.cat([c[:n + 2], c[n + 3:]]), torch.cat([lq[:n + 2], lq[n + 3:]]), x3=x3)
    assert float((lse - w[0]).abs().max()) <= 1e-5 * float(w[0].abs().max())  # as if the column were not there


@pytest.mark.parametrize("form", FORMS)
def test_weights_and_mining_compose(cuda, form):
    """(select,) rows, fold, cols_mixed against the fp64 restatement, as
    test_hard_neg_gpu.py::test_weights_compose does for the square case: the
    gap case (hard_neg_ref.gap_case) widened by 40 extra columns, the first 16
    along its directions u_g (one more negative near 2.25 for every row: K =
    9 keeps it, so mined dc is non-zero on extra columns), the rest near 0."""
    import hard_neg_ref as hn

    x3 = form == "x3"
    g = hn.gap_case()
    rng = np.random.default_rng(3)
    n, E, m, k = hn.GAP_N, hn.GAP_E, 40, hn.GAP_K + 1
    u = np.linalg.qr(np.random.default_rng(7).standard_normal((E, E)))[0][:16]  # gap_case's directions
    extra = 0.05 * rng.standard_normal((m, E))
    extra[:16] += 1.5 * u
    c = np.concatenate([g["c"], extra.astype(np.float32)])
    logq = np.concatenate([g["logq"], rng.uniform(-0.1, 0.0, m).astype(np.float32)])
    q, c, logq = (torch.as_tensor(v, device=cuda) for v in (g["q"], c, logq))
    sel = hn.select(hn.scores(q, c, logq, "fp64"), k)
    assert bool(((sel["a"] - sel["b"]) > 64 * hn.score_delta(q, c, form)).all())
    ref = hn.reference(q, c, logq, sel["kept"])
    w = torch.linspace(0.0, 1.0, n, device=cuda)
    tol = 1e-4 if x3 else 1e-3
    for kk, r in ((k, ref), (None, ir.reference_torch(q, c, logq))):
        wloss, dq, dc = losses.weighted_inbatch_grads(q, c, logq, w, x3=x3, num_hard_negatives=kk)
        want = float((w.double() * r["row_loss"]).sum())
        assert abs(float(wloss.double().sum()) - want) <= tol * abs(want), (kk, float(wloss.sum()), want)
        dq_ref = w.double()[:, None] * r["dq"]
        assert float((dq.double() - dq_ref).norm() / dq_ref.norm()) <= 10 * tol
        assert bool((dq[0] == 0).all())
        # dc of the weighted loss: sum_i w_i (P_ij - [j = i]) q_i, from the unweighted pieces
        S = hn.scores(q, c, logq, "fp64")
        rr = torch.arange(n, device=cuda)
        keep = torch.ones_like(S, dtype=torch.bool) if kk is None else sel["kept"].clone()
        keep[rr, rr] = True
        P = torch.softmax(S.masked_fill(~keep, float("-inf")), 1)
        P[rr, rr] -= 1.0
        dc_ref = (w.double()[:, None] * P).T @ q.double()
        assert tuple(dc.shape) == (n + m, E)
        assert float((dc.double() - dc_ref).norm() / dc_ref.norm()) <= 10 * tol, kk
        assert float(dc_ref[n:n + 16].norm()) > 0.1 * float(dc_ref.norm()) / np.sqrt(n + m)  # extra columns that matter
        assert float((dc.double()[n:] - dc_ref[n:]).norm() / dc_ref[n:].norm()) <= 10 * tol, kk
    # weights all one: the unweighted fused entry's values
    one = torch.ones_like(w)
    _, dq1, dc1 = losses.weighted_inbatch_grads(q, c, logq, one, x3=x3, num_hard_negatives=k)
    f = hip_ops.inbatch_fused_mixed(q, c, logq, x3=x3, hard_k=k)
    assert _bits(dq1, f[2]) and _bits(dc1, f[3])


def test_losses_accept_extra_negatives(cuda):
    """inbatch_softmax_xent / InBatchSoftmaxCrossEntropy with c longer than q:
    value and autograd gradients are the fused mixed entry's."""
    n, m, E = 130, 1, 48
    q, c, lq, ids = _dev(mn.case(n, m, E, hits=True), cuda)
    f = hip_ops.inbatch_fused_mixed(q, c, lq, ids=ids, loss_scale=1.0)
    ev = losses.inbatch_softmax_xent(q, c, lq, ids=ids)
    assert _bits(ev.reshape(1), hip_ops.loss_sum(f[1], 1.0).reshape(1))
    qg, cg = q.clone().requires_grad_(), c.clone().requires_grad_()
    loss = losses.InBatchSoftmaxCrossEntropy()(qg, cg, lq, ids)
    loss.backward()
    assert _bits(loss.detach().reshape(1), ev.reshape(1))
    assert _bits(qg.grad, f[2]) and _bits(cg.grad, f[3])


# --------------------------------------------------------------------------- the model
MB, MM, MN, ME, MH = 96, 40, 500, 32, 48
V = [str(i) for i in range(600)]


def _features():
    qf = [Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=16, vocab=V[:300]),
          Feature("post", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V[:50])]
    cf = [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=16, vocab=V),
          Feature("price", dtypes.float32, FeatureFamily.CANDIDATE),
          Feature("ptn", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=V[:20])]
    return qf, cf


def _catalogue(cuda):
    """N = 500 articles: embedding rows 101 .. 600 of "art" (rows 1 .. 100 are
    in no catalogue row; batches below use rows 0 .. 300)."""
    rng = np.random.default_rng(42)
    _, cf = _features()
    cols = {"art": np.arange(101, 101 + MN).astype(np.int32), "price": rng.uniform(0, 1, MN).astype(np.float32),
            "ptn": rng.integers(0, 21, MN).astype(np.int32)}
    return CandidateCatalogue(cols, cf, device=cuda)


def _model(cuda, seed=0, opt="adagrad", logq=True, cat=True, **kw):
    qf, cf = _features()
    rng = np.random.default_rng(seed)
    probs = {v: float(p) for v, p in zip(V, rng.dirichlet(np.ones(len(V))))} if logq else None
    m = TwoTowerModel(qf, cf, "art", ME, [MH], [MH], probs, device=cuda, seed=seed, **kw)
    m.compile(optimizer=OptimizerFactory.get_optimizer(opt, {"learning_rate": 0.05}))
    if cat:
        m.set_candidate_catalogue(_catalogue(cuda) if cat is True else cat)
    return m


def _batch(cuda, rng, n=MB):
    z = lambda v: torch.as_tensor(rng.integers(0, v, n).astype(np.int32), device=cuda)  # noqa: E731
    return {"cust": z(301), "post": z(51), "art": z(301), "ptn": z(21),
            "price": torch.as_tensor(rng.uniform(0, 1, n).astype(np.float32), device=cuda)}


def _state(m):
    out = {}
    for t, name in ((m.query_tower, "q"), (m.candidate_tower, "c")):
        out[name + ".mlp"] = t.dense.flat.detach().clone()
        for n, layer in t.input_layer.embedding_layers.items():
            out[f"{name}.{n}"] = layer.weight.detach().clone()
    return out


def _fp64_step(m, x, step, lr=0.05):
    """One mixed Adagrad step restated in torch fp64 with autograd: the B + M
    candidate batch built by hand from the numpy sampler; returns (loss,
    {name: updated parameter}, the sampled catalogue rows)."""
    cat = m.candidate_catalogue
    s = mn.sample(MM, cat.num_rows, m.sampled_negatives_seed, step)
    words = cat.words.cpu().numpy()
    cand = {}
    for i, name in enumerate(cat.feature_names):
        col = words[i, s]
        tail = torch.as_tensor(col.view(np.float32) if name == "price" else col, device=x[name].device)
        cand[name] = torch.cat([x[name], tail])
    params, outs = {}, []
    for t, tag, src in ((m.query_tower, "q", x), (m.candidate_tower, "c", cand)):
        layer = t.input_layer
        parts = [src[f.name].double()[:, None] for f in layer.numerical_features]
        for f in layer.categorical_features:
            w = layer.embedding_layers[f.name].weight.detach().double().clone().requires_grad_()
            params[f"{tag}.{f.name}"] = w
            parts.append(w[src[f.name].long()])
        h = torch.cat(parts, 1)
        flat = t.dense.flat.detach().double().clone().requires_grad_()
        params[f"{tag}.mlp"] = flat
        for w_off, fi, fo, _ in t.dense.layout:
            W = flat[w_off:w_off + fi * fo].view(fi, fo)
            b = flat[w_off + fi * fo:w_off + (fi + 1) * fo]
            h = torch.relu(h @ W + b)
        if m.normalize_embeddings:
            h = h / h.norm(dim=1, keepdim=True).clamp_min(1e-30)
        outs.append(h)
    qo, co = outs[0] / (m.temperature or 1.0), outs[1]
    S = qo @ co.T
    B = qo.shape[0]
    if m.logq_correction is not None:
        S = S - m.mixture_logq_table(B).double()[cand["art"].long()][None, :]
    rr = torch.arange(B, device=S.device)
    if m.remove_accidental_hits:
        hit = cand["art"][:B, None] == cand["art"][None, :]
        hit[rr, rr] = False
        S = S.masked_fill(hit, float("-inf"))
    loss = (torch.logsumexp(S, 1) - S[rr, rr]).sum()
    loss.backward()
    new = {}
    for k, p in params.items():  # Adagrad: acc = 0.1 + g^2; p -= lr g / (sqrt(acc) + eps); untouched rows: g = 0
        acc = 0.1 + p.grad ** 2
        new[k] = (p - lr * p.grad / (acc.sqrt() + 1e-7)).detach()
    return float(loss.detach()), new, s


@pytest.mark.parametrize("kw", [{}, {"remove_accidental_hits": True}], ids=["plain", "hits"])
def test_model_step_against_fp64(cuda, kw):
    """Loss within 1e-3 relative (test_hard_neg_gpu.py::test_model_loss_against_fp64)
    and every tensor's update within the first-step tolerances of
    tests/test_model_gpu.py (relative norm 1e-2 for an MLP buffer, 3e-3 for a
    table); a catalogue row that is in no batch has its embedding row
    changed."""
    m = _model(cuda, 4, num_sampled_negatives=MM, **kw)
    x = _batch(cuda, np.random.default_rng(6))
    x["art"][:5] = torch.as_tensor([150, 151, 152, 153, 154], dtype=torch.int32, device=cuda)  # also in the catalogue
    before = _state(m)
    want, new, s = _fp64_step(m, x, 0)
    got = float(m.train_step(x)["loss"])
    print(f"{kw}: loss {got:.6f}, fp64 {want:.6f}")
    assert abs(got - want) <= 1e-3 * abs(want)
    after = _state(m)
    for k in after:
        d_ref, d_gpu = new[k] - before[k].double(), after[k].double() - before[k].double()
        err = float((d_gpu - d_ref).norm() / d_ref.norm())
        print(f"first-step update {k}: rel err {err:.2e}")
        assert err <= (1e-2 if k.endswith("mlp") else 3e-3), (k, err)
    # the point of the feature: an article that only the sampler brought in moved
    art_rows = 101 + s
    only = [int(r) for r in art_rows if r > 300]
    assert only
    moved = (after["c.art"][only] != before["c.art"][only]).any(1)
    assert bool(moved.all())
    untouched = [r for r in range(301, 601) if r not in set(int(v) for v in art_rows)]
    assert torch.equal(after["c.art"][untouched], before["c.art"][untouched])
    assert int(m._mixed_step.item()) == 1 and int(m._mixed_status.item()) == 0
    # evaluation stays the plain in-batch loss
    plain = _model(cuda, 4, cat=False, **kw)
    for t, u in zip(plain.towers, m.towers):
        t.dense.flat.data.copy_(u.dense.flat.data)
        for name, layer in t.input_layer.embedding_layers.items():
            layer.weight.copy_(u.input_layer.embedding_layers[name].weight)
    assert torch.equal(m.compute_loss(x, training=False), plain.compute_loss(x, training=False))


@pytest.mark.parametrize("path", ["fused_optimizer_apply", "graphed", "device_fit"])
def test_model_step_forms_train_bit_identically(cuda, path):
    """Three steps (sampler steps 0, 1, 2): every form of the step leaves the
    eager step's state bit for bit and returns its losses."""
    rng = np.random.default_rng(8)
    batches = [_batch(cuda, rng) for _ in range(3)]
    a = _model(cuda, 5, num_sampled_negatives=MM, sampled_negatives_seed=11, remove_accidental_hits=True)
    want = [a.train_step(x)["loss"].clone() for x in batches]
    d = _model(cuda, 5, remove_accidental_hits=True)
    assert not torch.equal(d.train_step(batches[0])["loss"], want[0])  # and it is not the default step
    b = _model(cuda, 5, num_sampled_negatives=MM, sampled_negatives_seed=11, remove_accidental_hits=True,
               fused_optimizer_apply=path == "fused_optimizer_apply")
    if path == "graphed":
        g = GraphedTrainStep(b, batches[0], warmup=1)
        got = [g.warmup_out["loss"].clone()] + [g(x)["loss"].clone() for x in batches[1:]]
        assert g.reusable(b, batch=batches[0])
        b.set_candidate_catalogue(_catalogue(cuda))
        assert not g.reusable(b, batch=batches[0])  # captured with another catalogue
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
    assert int(a._mixed_step.item()) == 3
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (path, k)


def test_model_with_a_catalogue_and_no_m_is_the_default_step_bitwise(cuda):
    rng = np.random.default_rng(12)
    batches = [_batch(cuda, rng) for _ in range(2)]
    a, b = _model(cuda, 3, cat=False), _model(cuda, 3)
    assert b.candidate_catalogue is not None and b.num_sampled_negatives is None
    for x in batches:
        assert torch.equal(a.train_step(x)["loss"], b.train_step(x)["loss"])
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert int(b._mixed_step.item()) == 0


def test_model_every_option_together(cuda):
    """Adam, cosine scoring with a temperature, accidental hits, mining and
    sample weights in one mixed step: finite, the loss falls over a few steps
    on one batch, and the sampler advanced."""
    m = _model(cuda, 7, opt="adam", num_sampled_negatives=MM, remove_accidental_hits=True, normalize_embeddings=True,
               temperature=0.1, num_hard_negatives=16)
    x = _batch(cuda, np.random.default_rng(2))
    x["__weight__"] = torch.linspace(0.1, 1.0, MB, device=cuda)
    m.sample_weight_scale = 2.0
    ls = [float(m.train_step(x)["loss"]) for _ in range(6)]
    assert all(np.isfinite(ls)) and ls[-1] < ls[0], ls
    assert int(m._mixed_step.item()) == 6
    for v in _state(m).values():
        assert bool(torch.isfinite(v).all())
