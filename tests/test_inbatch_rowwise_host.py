"""CPU: the per-element checker of the in-batch loss (tests/inbatch_rowwise.py,
oracle.inbatch_reference / inbatch_bounds / inbatch_contract_bounds) is right
and sharp before any kernel is held to it:

  * the recipes do what they say (confident rows' pos - a over [5, 40], late
    maxima 9 .. 12 log2 units over what their rows streamed before, a combine
    whose other splits underflow);
  * the contract restatement lies within the certified bf16 bounds of the
    fp64 reference on every trained input set (certified rows);
  * the x3 bounds certify every row of every case; the small-score cases
    certify every row for bf16 too;
  * six injected kernel faults are each rejected per element, beside the
    whole-matrix norm the suite relied on so far (printed);
  * the cancellation-free reference equals oracle.inbatch_softmax_xent where
    that one does not cancel, and keeps a positive loss where it gives 0;
  * the torch twins equal the numpy functions.
"""
import numpy as np
import pytest
import torch

import inbatch_rowwise as ir
from oracle import oracle

# (B, E, scale, trained, hits); the small-score cases carry no duplicate candidates
ALL = [c + (True, h) for c in ir.TRAINED for h in (False, True)] + [c + (False, False) for c in ir.SMALL]


@pytest.mark.parametrize("B,E,scale", ir.TRAINED)
def test_recipes_reach_their_regimes(B, E, scale):
    x, ref = ir.reference(B, E, scale)
    m = x["marks"]
    d = ref["d"]
    conf = -d[m["confident"]]
    step = 35.0 / len(conf)  # the targets are evenly spaced over [5, 40]
    assert 4.9 <= conf.min() <= 5.1 + 2 * step and 40.1 >= conf.max() >= 39.9 - 2 * step, (conf.min(), conf.max())
    assert ref["row_loss"][m["confident"]].min() < 1e-15 and ref["row_loss"][m["confident"]].max() > 3e-3
    assert ref["row_loss"][m["lost"]].min() > 10.0
    p = ir.plan(B, B)
    assert ir.fused_plan(B)["per_split"] == p["per_split"]  # the plants sit alike in both entries' splits
    if B in (4100, 2080):
        assert p["split"] == 16 and p["tiles"] == (5 if B == 4100 else 3) and p["nonempty"] == (13 if B == 4100 else 11)
        g = ir.late_gaps(x)
        assert all(9.0 < v < 12.0 for v in g["late"]), g["late"]
        assert g["wave"].min() > 9.0 and g["wave"].max() < 12.0 and len(g["wave"]) >= 32
        tiles = {t for *_, t in m["late"]}
        assert tiles >= ({1, 2, 3, 4} if B == 4100 else {1, 2})
        r, col, s, t = m["late"][0]  # the tile after the one holding the row's positive
        assert (r // 64) + 1 == col // 64 and t >= 1
    if B == 2080:  # a plant in the last of four ranks' columns, for a row of another rank
        assert any(col >= 1560 and r < 1560 for r, col, *_ in m["late"])
    if m["underflow"]:
        assert ir.late_gaps(x)["underflow"] >= 150.0
        r, col = m["underflow"]
        others = np.delete(np.arange(B), [r, col])
        assert (others // p["per_split"] != col // p["per_split"]).sum() > 0.5 * B or p["tiles"] == 1
    else:
        assert p["nonempty"] < 3


@pytest.mark.parametrize("B,E,scale,trained,hits", ALL)
def test_restatement_within_the_certified_bf16_bounds(B, E, scale, trained, hits):
    """E.1: oracle.inbatch_softmax_xent_bf16 against inbatch_reference with the
    bf16 parameters; rows with alpha >= 0.25 left out (their count printed)."""
    x, ref = ir.reference(B, E, scale, trained, hits)
    bnd = ir.bounds(B, E, scale, trained, hits, "bf16")
    con, _ = ir.contract(B, E, scale, trained, hits)
    print(f"B={B} E={E}: {int((~bnd['certified']).sum())} of {B} rows uncertified for bf16 "
          f"(alpha max {bnd['alpha'].max():.3g})")
    bad = ir.violations(con, ref, bnd, d=ref["d"], tag=f"B={B} E={E} restatement")
    assert not bad, "\n".join(bad)


def test_rank_block_of_the_reference_and_restatement():
    """rows_q: rank 3 of 4 at B = 2080 (pos_offset 1560) is the full batch's
    block, and the restatement of that block holds the block's bounds."""
    B, E, scale = ir.TRAINED[1]
    x, ref = ir.reference(B, E, scale)
    sl = slice(1560, 2080)
    blk = oracle.inbatch_reference(x["q"][sl], x["c"], x["logq"], 1560, rows_q=x["q"])
    own = oracle.inbatch_reference(x["q"][sl], x["c"], x["logq"], 1560)
    for k in ("lse", "row_loss", "dq", "d", "g", "A"):
        np.testing.assert_array_equal(blk[k], ref[k][sl])
        np.testing.assert_allclose(own[k], ref[k][sl], rtol=1e-12, atol=1e-300)
    np.testing.assert_array_equal(blk["dc"], ref["dc"])
    con = oracle.inbatch_softmax_xent_bf16(x["q"][sl], x["c"], x["logq"], pos_offset=1560)
    bnd = oracle.inbatch_bounds(own, x["q"][sl], x["c"], *ir.FORMS["bf16"], n_rows_total=B)
    bad = ir.violations(con, own, bnd, d=own["d"], keys=("lse", "row_loss", "dq"), tag="rank 3")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("B,E,scale,trained,hits", ALL)
def test_every_row_is_certified_for_x3(B, E, scale, trained, hits):
    """E.2: alpha < 0.25 on every row with the x3 parameters; the small-score
    cases certify every row with the bf16 parameters as well."""
    bnd = ir.bounds(B, E, scale, trained, hits, "x3")
    assert bool(bnd["certified"].all()), float(bnd["alpha"].max())
    assert float(bnd["alpha"].max()) < 0.05
    if not trained:
        assert bool(ir.bounds(B, E, scale, trained, hits, "bf16")["certified"].all())


# --------------------------------------------------------------------------- E.3: the checker is sharp
def _outputs(Sn, pos, q, c, g_scale=None, wnum=None):
    """lse, row_loss, dq, dc from the negatives' scores Sn (-inf elsewhere) and
    the positives' pos; g_scale [R] multiplies g, wnum [R,C] the numerator
    weights of the mean (the faults' handles)."""
    mx = Sn.max(axis=1)
    e = np.exp(Sn - mx[:, None])
    L = e.sum(axis=1)
    a = mx + np.log(L)
    w = e / L[:, None]
    d = a - pos
    g = np.exp(-oracle._softplus(-d))
    if g_scale is not None:
        g = g * g_scale
    mean = (w if wnum is None else w * wnum) @ c
    dc = (w * g[:, None]).T @ q - g[:, None] * q
    return {"lse": np.logaddexp(a, pos), "row_loss": oracle._softplus(d), "dq": g[:, None] * (mean - c), "dc": dc,
            "g": g, "w": w}


@pytest.fixture(scope="module")
def sharp():
    """The B = 4100 trained inputs, plain and hits, as dense score matrices."""
    out = {}
    B, E, scale = ir.TRAINED[0]
    for hits in (False, True):
        x, ref = ir.reference(B, E, scale, True, hits)
        q, c, lq = (x[k].astype(np.float64) for k in ("q", "c", "logq"))
        S = q @ c.T - lq[None, :]
        pos = np.diag(S).copy()
        S[oracle._not_negative(0, B, B, 0, x["ids"], x["ids"])] = -np.inf
        base = _outputs(S, pos, q, c)
        for k in ("lse", "row_loss", "dq", "dc"):  # the dense form is the reference
            np.testing.assert_allclose(base[k], ref[k], rtol=1e-9, atol=1e-300)
        out[hits] = (x, ref, q, c, S, pos, base)
    return out


def _rejected(name, got, hits, keys, old_tol=None):
    """The faulted fp64 outputs `got` against the reference by the x3 bounds
    (section B) and, moved onto the restatement, by the contract bounds
    (section C); both must object.  Prints the whole-matrix figures."""
    B, E, scale = ir.TRAINED[0]
    x, ref = ir.reference(B, E, scale, True, hits)
    full = {k: got.get(k, ref[k]) for k in ("lse", "row_loss", "dq", "dc")}
    wm = ir.whole_matrix(full, ref)
    bad_b = ir.violations(full, ref, ir.bounds(B, E, scale, True, hits, "x3"), d=ref["d"], tag=name)
    con, cb = ir.contract(B, E, scale, True, hits)
    moved = {k: con[k].astype(np.float64) + (full[k] - ref[k]) for k in ("dq", "dc")}
    bad_c = ir.violations(moved, con, cb, d=ref["d"], keys=("dq", "dc"), tag=name + " (contract)")
    print(f"fault {name}: whole-matrix dq {wm[0]:.3e} dc {wm[1]:.3e}")
    print("\n".join(bad_b + bad_c))
    for k in keys:
        assert any(f" {k}:" in line for line in bad_b), (name, k, "section B does not object")
        assert any(f" {k}:" in line for line in bad_c), (name, k, "section C does not object")
    if old_tol is not None:  # the suite's tolerances so far would have let it pass
        assert max(wm) < old_tol, wm
    return wm


def test_fault_a_one_wave_skips_one_tile(sharp):
    x, ref, q, c, S, pos, base = sharp[False]
    S2 = S.copy()
    S2[320:352, 1280:1344] = -np.inf
    _rejected("(a) wave 10 skips tile 20", _outputs(S2, pos, q, c), False, ("dq", "dc"), old_tol=1e-3)


def test_fault_b_o_not_rescaled_at_a_late_maximum(sharp):
    """O of the tiles before the planted maximum keeps its old scale while L
    is rescaled: their numerator weights are 2^(m_new - m_old) too heavy."""
    x, ref, q, c, S, pos, base = sharp[False]
    per = x["marks"]["plan"]["per_split"]
    wnum = np.ones_like(S)
    for r, col, s, t in x["marks"]["late"]:
        before = slice(s * per, s * per + 64 * t)
        m_old, m_new = np.ceil(S[r, before].max() * ir.LOG2E), np.ceil(S[r, col] * ir.LOG2E)
        assert m_new - m_old >= 9
        wnum[r, before] = 2.0 ** (m_new - m_old)
    _rejected("(b) O not rescaled", _outputs(S, pos, q, c, wnum=wnum), False, ("dq",))


def test_fault_c_g_doubled_on_confident_rows(sharp):
    x, ref, q, c, S, pos, base = sharp[False]
    _rejected("(c) g doubled where a - pos < -5", _outputs(S, pos, q, c, g_scale=np.where(ref["d"] < -5.0, 2.0, 1.0)),
              False, ("dq", "dc"), old_tol=1e-3)


def test_fault_d_cols_pass_masks_the_next_column(sharp):
    x, ref, q, c, S, pos, base = sharp[False]
    B = len(q)
    dc = base["dc"].copy()
    dc += (1.0 - base["g"])[:, None] * q  # column i keeps its positive row: P_ii = 1 - g_i
    i = np.arange(B - 1)
    np.subtract.at(dc, i + 1, (base["g"][i] * base["w"][i, i + 1])[:, None] * q[i])  # and column i + 1 loses row i
    wm = _rejected("(d) cols pass masks column i + 1", {"dc": dc}, False, ("dc",))
    assert wm[0] == 0.0


def test_fault_e_a_hit_left_unmasked_on_a_confident_row(sharp):
    x, ref, q, c, S, pos, base = sharp[True]
    conf = set(x["marks"]["confident"].tolist())
    i, j = next((i, j) for i, j in x["marks"]["dups"] if i in conf and ref["d"][i] < -20.0)
    S2 = S.copy()
    S2[i, j] = q[i] @ c[j] - float(x["logq"][j])  # the duplicate scores what the positive scores
    assert abs(S2[i, j] - pos[i]) < 1e-9
    _rejected(f"(e) hit ({i}, {j}) unmasked", _outputs(S2, pos, q, c), True, ("dq", "dc"))


def test_fault_f_one_split_dropped_in_the_combine(sharp):
    x, ref, q, c, S, pos, base = sharp[False]
    per = x["marks"]["plan"]["per_split"]
    S2 = S.copy()
    S2[1600:1616, 6 * per:7 * per] = -np.inf  # the 16 rows of one combine block lose split 6
    _rejected("(f) split 6 dropped for rows 1600-1615", _outputs(S2, pos, q, c), False, ("dq", "dc"))


# --------------------------------------------------------------------------- E.4
def test_reference_agrees_with_the_oracle_where_that_does_not_cancel():
    B, E, scale = ir.SMALL[0]
    x, ref = ir.reference(B, E, scale, False)
    old = oracle.inbatch_softmax_xent(x["q"], x["c"], x["logq"])
    for k in ("lse", "row_loss", "dq", "dc"):
        np.testing.assert_allclose(ref[k], old[k], rtol=1e-9, atol=1e-13)
    B, E, scale = ir.TRAINED[1]
    x, ref = ir.reference(B, E, scale)
    old = oracle.inbatch_softmax_xent(x["q"], x["c"], x["logq"])
    np.testing.assert_allclose(ref["lse"], old["lse"], rtol=1e-12)
    big = ref["row_loss"] > 1e-3
    np.testing.assert_allclose(ref["row_loss"][big], old["row_loss"][big], rtol=1e-9)
    conf = x["marks"]["confident"]
    zero = old["row_loss"][conf] == 0.0
    print(f"lse - S_pos is exactly 0.0 on {int(zero.sum())} of {len(conf)} confident rows")
    assert zero.sum() > 0
    assert bool((ref["row_loss"][conf] > 0).all())
    # where the old form still has digits, the new loss is its value to those digits
    some = conf[(old["row_loss"][conf] > 1e-9)]
    np.testing.assert_allclose(ref["row_loss"][some], old["row_loss"][some], rtol=1e-5)


# --------------------------------------------------------------------------- twins
@pytest.mark.parametrize("B,E,scale,trained,hits", [ir.TRAINED[2] + (True, True), ir.SMALL[0] + (False, False)])
def test_torch_twins_equal_numpy(B, E, scale, trained, hits):
    x, ref = ir.reference(B, E, scale, trained, hits)
    t = {k: torch.from_numpy(x[k]) for k in ("q", "c", "logq")}
    ids = None if x["ids"] is None else torch.from_numpy(x["ids"])
    tref = ir.reference_torch(t["q"], t["c"], t["logq"], 0, ids, ids, block=50)
    for k in ("lse", "row_loss", "dq", "dc", "a", "d", "g", "n", "mean", "A"):
        np.testing.assert_allclose(tref[k].numpy(), ref[k], rtol=1e-10, atol=1e-300, err_msg=k)
    for form in ("x3", "bf16"):
        bnd = ir.bounds(B, E, scale, trained, hits, form)
        tb = ir.bounds_torch(tref, t["q"], t["c"], *ir.FORMS[form], block=50)
        for k in ("lse", "row_loss", "log_row_loss", "dq", "dc", "dc_pos", "alpha"):
            np.testing.assert_allclose(tb[k].numpy(), bnd[k], rtol=1e-9, atol=1e-300, err_msg=k)
        np.testing.assert_array_equal(tb["certified"].numpy(), bnd["certified"])
