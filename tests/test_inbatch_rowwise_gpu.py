"""The in-batch loss kernels per element, in the trained and wide-score
regimes (tests/inbatch_rowwise.py: signed operands, confident and lost rows,
late maxima for one lane and for a whole wave, a split combine whose other
splits underflow, logQ edges, duplicate candidates): the fused entry and
rows + cols at one and at four emulated ranks, each in the plain, hits, x3 and
x3-hits forms.  Every element of lse, row_loss, dq and dc is held to its own
bound (oracle.inbatch_bounds / inbatch_contract_bounds):

  x3 forms    against the cancellation-free fp64 reference, certified bounds
              with the x3 parameters; no row is left out;
  bf16 forms  against the contract restatement, its per-element residual; and
              against fp64 with the bf16 parameters on the cases where those
              certify every row (the count of uncertified rows is printed).

The plans (the smallest shapes that reach each path; inbatch_rowwise.TRAINED):
B = 4100: 16 splits of 5 tiles, the ring wraps; B = 2080: 16 splits of 3
tiles, empty splits, and 4 ranks of 520 rows with pos_offset > 0; B = 129 and
65: the last positive in a tile with one real row; B = 37: one ragged tile.
On failure each line names the worst row, element, ratio to bound and d_i.
"""
import numpy as np
import pytest
import torch

import inbatch_rowwise as ir
from oracle import oracle
from pkg.modelling import hip_ops

pytestmark = pytest.mark.gpu

FORMS = [("plain", False, False), ("hits", False, True), ("x3", True, False), ("x3-hits", True, True)]
# (B, E, scale, trained, entry); entry: "fused", or the number of emulated ranks of rows + cols
RUNS = [c + (True, e) for c in ir.TRAINED for e in ("fused", 1)] + [ir.TRAINED[1] + (True, 4)] \
    + [c + (False, e) for c in ir.SMALL for e in ("fused", 1)]

_DEV: dict = {}


def _setup(cuda, B, E, scale, trained, hits):
    """The case's tensors, its fp64 reference (torch twin on the device) and
    the reference as numpy, once per case."""
    key = (B, E, scale, trained, hits)
    if key not in _DEV:
        x = ir.case(B, E, scale, trained, hits)
        t = {k: torch.from_numpy(x[k]).to(cuda) for k in ("q", "c", "logq")}
        t["ids"] = None if x["ids"] is None else torch.from_numpy(x["ids"]).to(cuda)
        ref = ir.reference_torch(t["q"], t["c"], t["logq"], 0, t["ids"], t["ids"])
        _DEV[key] = (x, t, ref, ir.to_numpy(ref), {})
    return _DEV[key]


def _bounds(cuda, B, E, scale, trained, hits, form):
    x, t, ref, _, cache = _setup(cuda, B, E, scale, trained, hits)
    if form not in cache:
        cache[form] = ir.to_numpy(ir.bounds_torch(ref, t["q"], t["c"], *ir.FORMS[form]))
    return cache[form]


def _run(t, entry, x3, ids, **kw):
    """(lse, row_loss, dq, dc) of the whole batch through one entry."""
    q, c, logq = t["q"], t["c"], t["logq"]
    if entry == "fused":
        return hip_ops.inbatch_fused(q, c, logq, x3=x3, ids=ids, **kw)
    B = q.shape[0]
    b = B // entry
    assert b * entry == B
    sl = [slice(r * b, (r + 1) * b) for r in range(entry)]
    rk = lambda s: {} if ids is None else {"row_ids": ids[s], "col_ids": ids}  # noqa: E731
    ck = lambda s: {} if ids is None else {"row_ids": ids, "col_ids": ids[s]}  # noqa: E731
    rows = [hip_ops.inbatch_rows(q[s], c, logq, pos_offset=s.start, x3=x3, **rk(s)) for s in sl]
    lse, loss = torch.cat([o[0] for o in rows]), torch.cat([o[1] for o in rows])
    dc = torch.cat([hip_ops.inbatch_cols(q, lse, c[s], logq[s], pos_offset=s.start, row_loss=loss, x3=x3, **ck(s))
                    for s in sl])
    return lse, loss, torch.cat([o[2] for o in rows]), dc


def _named(out):
    return dict(zip(("lse", "row_loss", "dq", "dc"), out[:4]))


def check_outputs(cuda, out, B, E, scale, trained, hits, x3, tag):
    """The assertions of this module on one entry's outputs (see its docstring)."""
    x, t, ref, ref_np, _ = _setup(cuda, B, E, scale, trained, hits)
    got = _named(out)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (tag, k)
    bad = []
    if x3:
        bnd = _bounds(cuda, B, E, scale, trained, hits, "x3")
        assert bool(bnd["certified"].all()), (tag, float(bnd["alpha"].max()))
        bad += ir.violations(got, ref_np, bnd, d=ref_np["d"], tag=tag + " vs fp64 (x3 bounds)")
    else:
        con, cb = ir.contract(B, E, scale, trained, hits)
        bad += ir.violations(got, con, cb, d=ref_np["d"], tag=tag + " vs contract")
        bnd = _bounds(cuda, B, E, scale, trained, hits, "bf16")
        left_out = int((~bnd["certified"]).sum())
        print(f"{tag}: {left_out} of {B} rows uncertified against fp64 with the bf16 parameters"
              f"{'' if left_out else ': held to fp64 as well'}")
        if left_out == 0:
            bad += ir.violations(got, ref_np, bnd, d=ref_np["d"], tag=tag + " vs fp64 (bf16 bounds)")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("form,x3,hits", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("B,E,scale,trained,entry", RUNS)
def test_rowwise(cuda, B, E, scale, trained, entry, form, x3, hits):
    hits = hits and trained  # the small-score cases carry no duplicates: their hits forms run on distinct ids
    x, t, *_ = _setup(cuda, B, E, scale, trained, hits)
    ids = t["ids"]
    if form.endswith("hits") and ids is None:
        ids = torch.arange(B, dtype=torch.int32, device=cuda)
    out = _run(t, entry, x3, ids if form.endswith("hits") else None)
    check_outputs(cuda, out, B, E, scale, trained, hits, x3, f"{form} B={B} E={E} {entry}")


@pytest.mark.parametrize("x3,B,E,scale,trained", [(True,) + ir.TRAINED[1] + (True,), (True,) + ir.TRAINED[3] + (True,),
                                                  (False,) + ir.SMALL[0] + (False,)])
def test_cols_without_row_loss(cuda, x3, B, E, scale, trained):
    """inbatch_cols(row_loss=None) takes 1 - P_pos from -expm1(pos - lse) in
    fp32: once a row's loss is below ulp(lse) / 2 that is 0 where the exact
    value is the loss itself, so no relative bound holds; the absolute one
    does: |d(1 - P_pos)| <= 2^-23 (|pos| + |lse|) + delta' (fp32 rounding of
    pos, lse and their difference under a 1-Lipschitz map, and lse's own
    error), in place of the g_pos term of the dc bound."""
    x, t, ref, ref_np, _ = _setup(cuda, B, E, scale, trained, False)
    form = "x3" if x3 else "bf16"
    bnd = _bounds(cuda, B, E, scale, trained, False, form)
    assert bool(bnd["certified"].all())
    lse, row_loss, _ = hip_ops.inbatch_rows(t["q"], t["c"], t["logq"], x3=x3)
    dc = hip_ops.inbatch_cols(t["q"], lse, t["c"], t["logq"], x3=x3)
    omp = 2.0 ** -23 * (np.abs(ref_np["pos"]) + np.abs(ref_np["lse"])) + bnd["delta_pos"]
    wide = dict(bnd, dc=bnd["dc"] - bnd["dc_pos"] + omp[:, None] * np.abs(x["q"].astype(np.float64)))
    bad = ir.violations({"dc": dc}, ref_np, wide, keys=("dc",), tag=f"{form} B={B} cols without row_loss")
    assert not bad, "\n".join(bad)
    if trained:  # with row_loss the narrower g_pos term holds; both ratios printed for the confident rows
        with_loss = hip_ops.inbatch_cols(t["q"], lse, t["c"], t["logq"], row_loss=row_loss, x3=x3)
        assert not ir.violations({"dc": with_loss}, ref_np, bnd, keys=("dc",))
        conf = x["marks"]["confident"]
        tiny = conf[ref_np["row_loss"][conf] < 1e-9]
        err = np.abs(dc.double().cpu().numpy() - ref_np["dc"])[tiny]
        print(f"cols without row_loss: worst |d dc| / bound on rows with loss < 1e-9: "
              f"{float((err / bnd['dc'][tiny]).max()):.3g} (narrow bound), {float((err / wide['dc'][tiny]).max()):.3g}")


@pytest.mark.parametrize("form,x3,hits", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("B,E,scale,entry", [ir.TRAINED[0] + ("fused",), ir.TRAINED[1] + (4,)])
def test_reruns_are_bit_identical(cuda, B, E, scale, entry, form, x3, hits):
    """Twice on the late-maximum inputs (mid-stream rescales, underflowing
    combine weights): lse, row_loss, dq and dc bit for bit."""
    x, t, *_ = _setup(cuda, B, E, scale, True, hits)
    first = [o.clone() for o in _run(t, entry, x3, t["ids"])]
    torch.cuda.synchronize()
    again = _run(t, entry, x3, t["ids"])
    for n, a, b in zip(("lse", "row_loss", "dq", "dc"), first, again):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("form,x3,hits", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("B,E,scale", [ir.TRAINED[0], ir.TRAINED[3]])
def test_loss_in_launch_on_confident_rows(cuda, B, E, scale, form, x3, hits):
    """loss_scale= on the confident inputs (row losses from 1e-17 to tens in
    one sum): still loss_sum(row_loss) bit for bit, the other outputs
    unchanged."""
    x, t, *_ = _setup(cuda, B, E, scale, True, hits)
    want = _run(t, "fused", x3, t["ids"])
    got = _run(t, "fused", x3, t["ids"], loss_scale=0.25)
    assert torch.equal(got[4], hip_ops.loss_sum(got[1], 0.25))
    for n, a, b in zip(("lse", "row_loss", "dq", "dc"), want, got[:4]):
        assert torch.equal(a, b), n
