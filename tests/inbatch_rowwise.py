"""Per-element checks of the in-batch loss kernels (csrc/tt_inbatch.hip),
shared by tests/test_inbatch_rowwise_host.py and tests/test_inbatch_rowwise_gpu.py
and called from the older in-batch tests:

  plan() / fused_plan()   the launch plans of make_plan / fused_plan, restated
  case()                  deterministic inputs in the trained and wide-score
                          regimes (signed operands, confident / lost rows, late
                          maxima, a split combine that underflows, logQ edges,
                          duplicate candidates for the hits forms)
  reference_torch() / bounds_torch()
                          torch fp64 twins of oracle.inbatch_reference /
                          oracle.inbatch_bounds (same formulas; on the device
                          they cost milliseconds where numpy costs seconds)
  violations()            the checker: every element of lse, row_loss, dq and
                          dc against its own bound

The bounds themselves are derived in oracle.inbatch_bounds and
oracle.inbatch_contract_bounds.
"""
import functools
import math

import numpy as np

from oracle import oracle

LOG2E = 1.4426950408889634
K_TILE, K_ROWS_WG, K_MAX_SPLIT, K_WG_TARGET = 64, 128, 16, 512  # csrc/tt_inbatch.hip


def _round_up(x, m):
    return (x + m - 1) // m * m


def plan(n_stat, n_strm):
    """make_plan of csrc/tt_inbatch.hip (the rows / cols entries):
    dict(stat_pad, strm_pad, split, per_split, tiles) with tiles = streamed
    tiles per split; splits past ceil(strm_pad / per_split) are empty."""
    stat_pad, strm_pad = _round_up(max(n_stat, 1), K_ROWS_WG), _round_up(max(n_strm, 1), K_TILE)
    s = max(1, min(-(-K_WG_TARGET // (stat_pad // K_ROWS_WG)), strm_pad // K_TILE, K_MAX_SPLIT))
    per = _round_up(-(-strm_pad // s), K_TILE)
    return {"stat_pad": stat_pad, "strm_pad": strm_pad, "split": s, "per_split": per, "tiles": per // K_TILE,
            "nonempty": -(-strm_pad // per)}


def fused_plan(n):
    """fused_plan (the single-device entry: both extents padded to 128)."""
    n_pad = _round_up(max(n, 1), K_ROWS_WG)
    return plan(n_pad, n_pad)


# --------------------------------------------------------------------------- inputs
def _neg_scores(q, c, logq, rows, ids):
    """fp64 scores of `rows` against every column, -inf off their negatives."""
    S = q[rows] @ c.T - logq[None, :]
    if ids is not None:
        S[ids[rows][:, None] == ids[None, :]] = -np.inf
    S[np.arange(len(rows)), rows] = -np.inf
    return S


@functools.lru_cache(maxsize=None)
def case(B, E, scale, trained=True, hits=False):
    """Inputs [B, E] for one shape: dict(q, c, logq (float32), ids (int32 or
    None), marks).  Signed N(0, scale^2) operands, logq ~ log U(1e-6, 1e-2),
    columns 5, 1029, ... logq = 0 and 69, 1093, ... log(1e-8) (a handful: each
    log(1e-8) column outweighs ~1000 ordinary ones in every row's softmax).  trained:
      confident  every second row: c_i = 2 q_i before q_i is scaled by lambda_i
                 (so c_i = kappa_i q_i, kappa_i = 2 / lambda_i), lambda_i solved
                 per row so that pos - a is spread evenly over [5, 40] (loss
                 1e-2 .. 1e-17).  The query's norm carries the confidence: the
                 row's own scores widen, the other rows' do not (kappa q_i with
                 kappa > 1 would make column i a strong negative of every row,
                 and pos - a could not pass ~ E / 2 - 14).
      lost       every fourth row (i % 4 == 1): c_i = -2 q_i, loss of tens.
      late maximum (where a split streams >= 2 tiles; marks["late"] = (row,
                 col, split, tile in split)): column col is raised along q_row
                 to 10.5 log2 units above everything the row streamed before it
                 in that split — one row of a wave; marks["wave"] = (rows, col,
                 ...): all of the rows [w0, w1) at once, which share the
                 component beta e (and little else), through c_col = gamma e.
      underflow  marks["underflow"] = (row, col): one row (q scaled by 8) whose
                 planted negative, in a late split, stands >= 150 log2 units
                 over every other score of the row: exp2f(m[u] - M) = 0 for
                 every other split of the combine.
    hits: ids = arange(B) but for ids[i + 7] = ids[i], c[i + 7] = c[i],
    logq[i + 7] = logq[i] at i = 0, 16, 32, ...: a confident row's duplicate
    scores exactly the positive's score (marks["dups"] = [(i, i + 7)])."""
    rng = np.random.default_rng(B * 131 + E)
    q = rng.standard_normal((B, E)) * scale
    c = rng.standard_normal((B, E)) * scale
    logq = np.log(rng.uniform(1e-6, 1e-2, B))
    j = np.arange(B)
    logq[j % 1024 == 5] = 0.0
    logq[j % 1024 == 69] = math.log(1e-8)
    marks = {"late": [], "wave": None, "underflow": None, "dups": [], "confident": np.zeros(0, int),
             "lost": np.zeros(0, int)}
    ids = None
    if not trained:
        return {"q": q.astype(np.float32), "c": c.astype(np.float32), "logq": logq.astype(np.float32), "ids": None,
                "marks": marks}
    p = plan(B, B)  # per_split is the fused entry's as well at every B used here
    per, T, ne = p["per_split"], p["tiles"], p["nonempty"]
    col_of = lambda s, t: s * per + K_TILE * t + 3  # noqa: E731  (3 mod 16: no confident, lost or duplicate column)
    late, wave, under = [], None, None
    if T >= 2:
        # (split, tile in split, row): the first row's positive sits in the tile before its plant
        spec = [(1, 1, per + 11), (3, T - 1, 27), (min(9, ne - 2), 1, (B // 2 // 16) * 16 - 5)]
        if T >= 4:
            spec += [(5, 2, 1035), (7, 3, 2059)]
        late = [(r, col_of(s, t), s, t) for s, t, r in spec]
        w0 = (B * 3 // 4) // 32 * 32
        # 2080: rows 1592 .. 1631 hold a whole wave of the one-rank launch (1600 ..) and of rank 3 of 4 (1592 ..)
        w0, w1 = (1592, 1632) if B == 2080 else (w0, w0 + 32)
        wave = (w0, w1, col_of(2, min(2, T - 1)), 2, min(2, T - 1))
    if ne >= 3:
        under = ((B * 7 // 8) // 16 * 16 + 11, col_of(ne - 1, 0))
        if under[1] >= B:
            under = (under[0], col_of(ne - 2, 0))
    special_rows = {r for r, *_ in late} | ({under[0]} if under else set()) \
        | (set(range(wave[0], wave[1])) if wave else set())
    assert all(r % 16 == 11 for r, *_ in late) and (not under or under[0] % 16 == 11), (late, under)
    # the wave's rows share 4 e and keep 0.1 of the rest: their scores differ little
    if wave:
        e = rng.standard_normal(E)
        e /= np.linalg.norm(e)
        w = slice(wave[0], wave[1])
        q[w] = 0.1 * (q[w] - (q[w] @ e)[:, None] * e[None, :]) + 4.0 * e[None, :]
    if under:
        q[under[0]] *= 8.0
    conf = np.array([i for i in range(0, B, 2) if i not in special_rows])
    lost = np.arange(1, B, 4)
    c[0::2] = 2.0 * q[0::2]
    c[lost] = -2.0 * q[lost]
    if hits:
        ids = np.arange(B, dtype=np.int32)
        for i in range(0, B - 7, 16):
            c[i + 7], logq[i + 7], ids[i + 7] = c[i], logq[i], ids[i]
            marks["dups"].append((i, i + 7))
    # plants, on the final columns before them (later plants sit in later splits)
    for r, col, s, t in late:
        S = _neg_scores(q, c, logq, np.array([r]), ids)[0]
        before = S[s * per:s * per + K_TILE * t].max()
        c[col] += (before + 10.5 / LOG2E - S[col]) * q[r] / (q[r] @ q[r])
    if wave:
        w0, w1, col, s, t = wave
        rows = np.arange(w0, w1)
        S = _neg_scores(q, c, logq, rows, ids)
        before = S[:, s * per:s * per + K_TILE * t].max(axis=1)
        c[col] = (before.max() + 9.5 / LOG2E + logq[col]) / 4.0 * e
    if under:
        r, col = under
        S = _neg_scores(q, c, logq, np.array([r]), ids)[0]
        c[col] += (np.delete(S, col).max() + 155.0 / LOG2E - S[col]) * q[r] / (q[r] @ q[r])
    # confident rows: lambda_i by Newton's iteration on the row's own pos - a.  a(lambda) is convex (a
    # log-sum-exp of scores linear in lambda), so d = pos - a is concave and, the positive outscoring every
    # negative per unit of lambda, increasing: from lambda = 0 (d < 0) the iterates rise to the root from below.
    target = np.linspace(5.0, 40.0, len(conf))[np.random.default_rng(B).permutation(len(conf))]
    lam = np.zeros(len(conf))
    for b0 in range(0, len(conf), 1024):
        rows = conf[b0:b0 + 1024]
        S1 = q[rows] @ c.T
        pos1 = S1[np.arange(len(rows)), rows].copy()
        mask = np.zeros_like(S1, bool)
        if ids is not None:
            mask = ids[rows][:, None] == ids[None, :]
        mask[np.arange(len(rows)), rows] = True
        S1[mask] = 0.0
        assert bool((pos1[:, None] > S1).all())
        bias = np.where(mask, -np.inf, -logq[None, :])
        x = np.zeros(len(rows))
        for _ in range(12):
            Z = x[:, None] * S1 + bias
            m = Z.max(axis=1)
            ez = np.exp(Z - m[:, None])
            L = ez.sum(axis=1)
            d = x * pos1 - logq[rows] - (m + np.log(L))
            x = x + (target[b0:b0 + 1024] - d) / (pos1 - (ez * S1).sum(axis=1) / L)
        lam[b0:b0 + 1024] = x
    q[conf] *= lam[:, None]
    marks.update(late=late, wave=wave, underflow=under, confident=conf, lost=lost, plan=p)
    return {"q": q.astype(np.float32), "c": c.astype(np.float32), "logq": logq.astype(np.float32), "ids": ids,
            "marks": marks}


def late_gaps(x):
    """log2 gaps of the planted maxima over what their rows streamed before in
    the split: dict(late=[gap], wave=[gaps of the rows], underflow=gap over
    every other negative of the row)."""
    q, c, logq = (x[k].astype(np.float64) for k in ("q", "c", "logq"))
    m = x["marks"]
    per = m["plan"]["per_split"]
    out = {"late": [], "wave": None, "underflow": None}
    for r, col, s, t in m["late"]:
        S = _neg_scores(q, c, logq, np.array([r]), x["ids"])[0]
        out["late"].append(float((S[col] - S[s * per:s * per + K_TILE * t].max()) * LOG2E))
    if m["wave"]:
        w0, w1, col, s, t = m["wave"]
        S = _neg_scores(q, c, logq, np.arange(w0, w1), x["ids"])
        out["wave"] = (S[:, col] - S[:, s * per:s * per + K_TILE * t].max(axis=1)) * LOG2E
    if m["underflow"]:
        r, col = m["underflow"]
        S = _neg_scores(q, c, logq, np.array([r]), x["ids"])[0]
        out["underflow"] = float((S[col] - np.delete(S, col).max()) * LOG2E)
    return out


# --------------------------------------------------------------------------- torch twins
def _softplus_t(x):
    import torch

    return torch.where(x > 0, x + torch.log1p(torch.exp(-x.abs())), torch.log1p(torch.exp(torch.clamp(x, max=0.0))))


def _not_negative_t(r0, r1, C, off, row_ids, col_ids, dev):
    import torch

    rr = torch.arange(r0, r1, device=dev)
    if row_ids is None:
        ex = torch.zeros(r1 - r0, C, dtype=torch.bool, device=dev)
    else:
        ex = row_ids[r0:r1, None] == col_ids[None, :]
    ex[rr - r0, rr + off] = True
    return ex


def reference_torch(q, c, logq=None, pos_offset=0, row_ids=None, col_ids=None, block=1024):
    """oracle.inbatch_reference on torch fp64 tensors of q's device (the same
    formulas line by line; dict of torch tensors)."""
    import torch

    q, c = q.double(), c.double()
    dev = q.device
    R, E = q.shape
    C = c.shape[0]
    lq = torch.zeros(C, dtype=torch.float64, device=dev) if logq is None else logq.double()
    out = {k: torch.zeros(R, dtype=torch.float64, device=dev) for k in ("row_loss", "lse", "a", "pos", "d", "g", "n")}
    out.update({k: torch.zeros(R, E, dtype=torch.float64, device=dev) for k in ("dq", "mean", "A", "cpos")})
    dc = torch.zeros(C, E, dtype=torch.float64, device=dev)
    ninf = torch.tensor(float("-inf"), dtype=torch.float64, device=dev)
    for r0 in range(0, R, block):
        r1 = min(R, r0 + block)
        b = slice(r0, r1)
        rr = torch.arange(r0, r1, device=dev)
        S = q[b] @ c.T - lq[None, :]
        pos = S[rr - r0, rr + pos_offset].clone()
        ex = _not_negative_t(r0, r1, C, pos_offset, row_ids, col_ids, dev)
        S = S.masked_fill(ex, float("-inf"))
        mx = S.max(dim=1).values
        none = ~torch.isfinite(mx)
        mx = torch.where(none, torch.zeros_like(mx), mx)
        e = torch.exp(S - mx[:, None])
        L = e.sum(dim=1)
        one = torch.ones_like(L)
        a = torch.where(none, ninf, mx + torch.log(torch.where(none, one, L)))
        w = e / torch.where(none, one, L)[:, None]
        d = torch.where(none, ninf, a - pos)
        dz = torch.where(none, torch.zeros_like(d), d)
        g = torch.where(none, torch.zeros_like(d), torch.exp(-_softplus_t(-dz)))
        cpos = c[rr + pos_offset]
        out["row_loss"][b] = torch.where(none, torch.zeros_like(d), _softplus_t(dz))
        out["lse"][b] = torch.where(none, pos, torch.logaddexp(torch.where(none, pos, a), pos))
        out["a"][b], out["pos"][b], out["d"][b], out["g"][b] = a, pos, d, g
        out["n"][b] = (~ex).sum(dim=1).double()
        out["mean"][b], out["A"][b], out["cpos"][b] = w @ c, w @ c.abs(), cpos
        out["dq"][b] = g[:, None] * (out["mean"][b] - cpos)
        dc += (w * g[:, None]).T @ q[b]
        dc[rr + pos_offset] -= g[:, None] * q[b]
    out.update(dc=dc, loss=float(out["row_loss"].sum()), logq=None if logq is None else lq, pos_offset=pos_offset,
               row_ids=row_ids, col_ids=col_ids)
    return out


def bounds_torch(ref, q, c, eps, u, n_rows_total=None, block=1024):
    """oracle.inbatch_bounds on torch fp64 tensors (ref from reference_torch)."""
    import torch

    q, c = q.double(), c.double()
    dev = q.device
    R, E = q.shape
    C = c.shape[0]
    Rt = R if n_rows_total is None else n_rows_total
    off, row_ids, col_ids = ref["pos_offset"], ref["row_ids"], ref["col_ids"]
    lq = torch.zeros(C, dtype=torch.float64, device=dev) if ref["logq"] is None else ref["logq"]
    aq, ac = q.abs(), c.abs()
    sigma = oracle.SOFTMAX_SLACK * (1.0 + ref["lse"].abs())
    delta = torch.empty(R, dtype=torch.float64, device=dev)
    delta_p = torch.empty_like(delta)
    dc_b = torch.zeros(C, E, dtype=torch.float64, device=dev)
    dc_pos = torch.zeros_like(dc_b)
    for r0 in range(0, R, block):
        r1 = min(R, r0 + block)
        b = slice(r0, r1)
        rr = torch.arange(r0, r1, device=dev)
        D = eps * (aq[b] @ ac.T)
        ex = _not_negative_t(r0, r1, C, off, row_ids, col_ids, dev)
        delta[b] = D.masked_fill(ex, 0.0).max(dim=1).values + sigma[b]
        delta_p[b] = delta[b] + E * 2.0 ** -24 * D[rr - r0, rr + off] / eps
        P = torch.exp(q[b] @ c.T - lq[None, :] - ref["lse"][b, None]).masked_fill(ex, 0.0)
        F = torch.exp(D + delta[b, None]) * (1.0 + u) ** 2 - 1.0 + Rt * 2.0 ** -24
        dc_b += (P * F).T @ aq[b]
        dc_pos[rr + off] += (ref["g"][b] * torch.expm1(delta_p[b]))[:, None] * aq[b]
    dc_b += dc_pos + 2.0 ** -21 * ref["dc"].abs() + oracle.FP32_TINY * (1.0 + aq.sum(dim=0))[None, :]
    alpha = torch.exp(delta) * (1.0 + u) ** 2 - 1.0 + ref["n"] * 2.0 ** -24
    cert = alpha < oracle.ALPHA_CAP
    al = torch.where(cert, alpha, torch.zeros_like(alpha))
    g = ref["g"]
    dq_b = (g * torch.exp(delta_p) * 2.0 * al / (1.0 - al))[:, None] * ref["A"] \
        + (g * torch.expm1(delta_p))[:, None] * (ref["mean"] - ref["cpos"]).abs() + 2.0 ** -21 * ref["dq"].abs() \
        + oracle.FP32_TINY * (1.0 + (ref["mean"] - ref["cpos"]).abs() + (ref["n"] * ac.max())[:, None])
    dq_b[~cert] = float("inf")
    return {"lse": delta_p + 2.0 ** -23 * ref["lse"].abs(), "row_loss": delta_p, "log_row_loss": delta_p + 2.0 ** -21,
            "dq": dq_b, "dc": dc_b, "dc_pos": dc_pos, "alpha": alpha, "certified": cert, "delta": delta,
            "delta_pos": delta_p}


def to_numpy(d):
    """A dict of the twins' results with every tensor as a numpy array."""
    return {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else v) for k, v in d.items()}


# --------------------------------------------------------------------------- the checker
def _np64(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, np.float64)


def violations(got, ref, bnd, d=None, keys=("lse", "row_loss", "dq", "dc"), tag=""):
    """Every element of got[k] (k in keys; arrays or tensors shaped as ref[k])
    against ref[k] within bnd[k]; row_loss also by |ln got - ln ref| <=
    bnd["log_row_loss"] where ref >= 1e-30 (got <= 2e-30 below that).  Rows
    with bnd["certified"] False are left out.  Returns one line per quantity
    that is over: count, worst ratio to its bound, its row, element and the
    row's d_i = a_i - pos_i (an empty list: everything holds)."""
    bad = []
    cert = np.asarray(bnd["certified"], bool) if "certified" in bnd else None
    dd = None if d is None else _np64(d)

    def over(name, err, bound, by_row):
        err, bound = np.asarray(err), np.broadcast_to(np.asarray(bound), np.shape(err))
        okrow = np.ones(err.shape[0], bool) if (cert is None or not by_row) else cert
        viol = (err > bound) | ~np.isfinite(err)
        viol &= okrow.reshape((-1,) + (1,) * (err.ndim - 1))
        if not viol.any():
            return
        ratio = np.where(viol, err / np.maximum(bound, 1e-300), 0.0)
        ratio = np.where(np.isfinite(ratio), ratio, np.inf)
        at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        drow = "" if dd is None or not by_row else f", d_i {dd[at[0]]:.4g}"
        bad.append(f"{tag} {name}: {int(viol.sum())} of {viol.size} over; worst at {tuple(int(a) for a in at)} "
                   f"err {err[at]:.4g} bound {bound[at]:.4g} (x{ratio[at]:.3g}){drow}")

    for k in keys:
        g, r = _np64(got[k]), _np64(ref[k])
        assert g.shape == r.shape, (k, g.shape, r.shape)
        over(k, np.abs(g - r), _np64(bnd[k]), by_row=k != "dc")
        if k == "row_loss":
            big = r >= 1e-30
            with np.errstate(divide="ignore", invalid="ignore"):
                lerr = np.where(big, np.abs(np.log(np.where(g > 0, g, np.nan)) - np.log(np.where(big, r, 1.0))), 0.0)
            lerr = np.where(big & ~(g > 0), np.inf, lerr)
            over("ln row_loss", lerr, _np64(bnd["log_row_loss"]), True)
            over("row_loss below 1e-30", np.where(big, 0.0, g), np.full(r.shape, 2e-30), True)
    return bad


def whole_matrix(got, ref):
    """The old metric: (||dq - ref|| / ||ref||, ||dc - ref|| / ||ref||)."""
    return tuple(float(np.linalg.norm(_np64(got[k]) - _np64(ref[k])) / max(np.linalg.norm(_np64(ref[k])), 1e-300))
                 for k in ("dq", "dc"))


# --------------------------------------------------------------------------- shared cases
# (B, E, scale) of the trained recipes; the plans (rows entry / fused entry, kMaxSplit = 16):
#   4100: stat_pad 4224 (33 workgroups), 65 / 66 streamed tiles, 16 splits of 5 tiles (13 / 14 hold
#         tiles): the ring wraps, a split holds stages 0-3 and a reuse
#   2080: stat_pad 2176 (17 workgroups), 33 / 34 tiles, 16 splits of 3 tiles, 5 / 4 of them empty;
#         4 ranks of 520 rows: stat_pad 640, the same 16 splits of 3 tiles, pos_offset 520 r
#   129:  3 / 4 tiles, one per split; the positive of row 128 in a tile with one real row
#   65:   2 tiles, one per split; the positive of row 64 likewise
#   37:   one ragged tile (the fused entry adds a fully padded second one)
TRAINED = [(4100, 64, 0.35), (2080, 128, 0.25), (129, 37, 0.45), (65, 16, 0.6), (37, 128, 0.25)]
# ordinary signed operands at max|S| <= 16: every row certified for the bf16 forms too
SMALL = [(300, 64, 0.15), (129, 100, 0.1)]
FORMS = {"x3": (oracle.X3_DOT_EPS, oracle.X3_P_U), "bf16": (oracle.BF16_DOT_EPS, oracle.BF16_P_U)}


@functools.lru_cache(maxsize=None)
def reference(B, E, scale, trained=True, hits=False):
    """(case, oracle.inbatch_reference of it), once per case."""
    x = case(B, E, scale, trained, hits)
    return x, oracle.inbatch_reference(x["q"], x["c"], x["logq"], 0, x["ids"], x["ids"])


@functools.lru_cache(maxsize=None)
def bounds(B, E, scale, trained=True, hits=False, form="x3"):
    x, ref = reference(B, E, scale, trained, hits)
    return oracle.inbatch_bounds(ref, x["q"], x["c"], *FORMS[form])


@functools.lru_cache(maxsize=None)
def contract(B, E, scale, trained=True, hits=False):
    """(restatement with aux, oracle.inbatch_contract_bounds of it)."""
    x = case(B, E, scale, trained, hits)
    con = oracle.inbatch_softmax_xent_bf16(x["q"], x["c"], x["logq"], row_ids=x["ids"], col_ids=x["ids"], aux=True)
    return con, oracle.inbatch_contract_bounds(con)


# --------------------------------------------------------------------------- for the older in-batch tests
def check_x3(out, q, c, logq, ids=None, tag="x3"):
    """An x3 entry's (lse, row_loss, dq, dc) on the device tensors q, c, logq
    (ids: the hits form) against the fp64 reference per element, by the
    certified x3 bounds; every row must be certified.  Returns violations()."""
    ref = reference_torch(q, c, logq, 0, ids, ids)
    bnd = to_numpy(bounds_torch(ref, q, c, *FORMS["x3"]))
    assert bool(bnd["certified"].all()), (tag, float(bnd["alpha"].max()))
    ref = to_numpy(ref)
    return violations(dict(zip(("lse", "row_loss", "dq", "dc"), out[:4])), ref, bnd, d=ref["d"], tag=tag)


def check_bf16(out, q, c, logq, con, ids=None, tag="bf16"):
    """A bf16 entry's outputs against its contract restatement `con`
    (oracle.inbatch_softmax_xent_bf16(..., aux=True) of the same inputs) per
    element, and against fp64 by the certified bf16 bounds where those certify
    every row (the count of uncertified rows is printed)."""
    got = dict(zip(("lse", "row_loss", "dq", "dc"), out[:4]))
    ref = reference_torch(q, c, logq, 0, ids, ids)
    bnd = to_numpy(bounds_torch(ref, q, c, *FORMS["bf16"]))
    ref = to_numpy(ref)
    bad = violations(got, con, oracle.inbatch_contract_bounds(con), d=ref["d"], tag=tag + " vs contract")
    left_out = int((~bnd["certified"]).sum())
    print(f"{tag}: {left_out} of {len(ref['d'])} rows uncertified against fp64 with the bf16 parameters")
    if left_out == 0:
        bad += violations(got, ref, bnd, d=ref["d"], tag=tag + " vs fp64")
    return bad
