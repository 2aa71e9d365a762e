"""Restatements for the sample-weight tests (numpy / torch on the CPU).

fold():           tt_inbatch_weight_rows' three per-row scalars, in fp32 (the
                  kernel's arithmetic, libm aside) or fp64.
scale_rows():     its in-place scaling of dq.
cols_formula():   the cols pass's formula in fp64, reading lse and row_loss
                  exactly where combine_cols_kernel reads them.
weighted_ref():   the weighted loss and its gradients by torch fp64 autograd on
                  S' = q.c^T - logq, accidental hits masked to -inf.
"""
import numpy as np
import torch


def fold(w, lse, row_loss, dtype=np.float32):
    """(lse_w, row_loss_w, wloss) per include/tt.h: copies at w == 1, (+inf,
    +0, +0) at w == 0, the formulas in between, NaN for a weight outside
    [0, 1]."""
    w = np.asarray(w, dtype)
    lse = np.asarray(lse, dtype)
    row_loss = np.asarray(row_loss, dtype)
    with np.errstate(all="ignore"):
        mid = (w > 0) & (w < 1)
        safe = np.where(mid, w, dtype(0.5))
        lse_w = np.where(mid, lse - np.log(safe), dtype(np.nan))
        row_loss_w = np.where(mid, -np.log1p(safe * np.expm1(-row_loss)), dtype(np.nan))
        wloss = np.where(mid, safe * row_loss, dtype(np.nan))
    one, zero = w == 1, w == 0
    lse_w = np.where(one, lse, np.where(zero, dtype(np.inf), lse_w)).astype(dtype)
    row_loss_w = np.where(one, row_loss, np.where(zero, dtype(0), row_loss_w)).astype(dtype)
    wloss = np.where(one, row_loss, np.where(zero, dtype(0), wloss)).astype(dtype)
    return lse_w, row_loss_w, wloss


def scale_rows(w, dq):
    """dq after the fold: row i times w_i (one multiply per element), stored
    as +0 at w_i == 0, left alone at w_i == 1, NaN for an invalid weight."""
    w = np.asarray(w, dq.dtype)
    out = dq.copy()
    with np.errstate(all="ignore"):
        mid = (w > 0) & (w < 1)
        out[mid] = dq[mid] * w[mid, None]
    out[w == 0] = 0
    out[~((w >= 0) & (w <= 1))] = np.nan
    return out


def cols_formula(Q, lse, row_loss, c_local, logq_local=None, pos_offset=0, row_ids=None, col_ids=None):
    """dc [C, E] in fp64: sum_{i != r(j)} exp(S'_ij - lse_i) q_i -
    (-expm1(-row_loss_r)) q_r with r(j) = j + pos_offset; accidental hits
    (row_ids[i] == col_ids[j], i != r(j)) are no pairs at all."""
    Q = np.asarray(Q, np.float64)
    c_local = np.asarray(c_local, np.float64)
    lse = np.asarray(lse, np.float64)
    row_loss = np.asarray(row_loss, np.float64)
    C = c_local.shape[0]
    S = Q @ c_local.T
    if logq_local is not None:
        S = S - np.asarray(logq_local, np.float64)[None, :]
    with np.errstate(all="ignore"):
        P = np.exp(S - lse[:, None])
    pos = np.zeros_like(P, dtype=bool)
    pos[pos_offset + np.arange(C), np.arange(C)] = True
    if row_ids is not None:
        P[(np.asarray(row_ids)[:, None] == np.asarray(col_ids)[None, :]) & ~pos] = 0.0
    P[pos] = np.expm1(-row_loss[pos_offset:pos_offset + C])  # = -(1 - P_rr) (times w_r once folded)
    return P.T @ Q


def weighted_ref(q, c, logq=None, w=None, ids=None):
    """fp64 autograd: dict(loss, row_loss, lse, dq, dc) of L = sum_i w_i l_i
    (w=None: all ones); row_loss and lse are the UNWEIGHTED per-row values."""
    tq = torch.tensor(np.asarray(q, np.float64), requires_grad=True)
    tc = torch.tensor(np.asarray(c, np.float64), requires_grad=True)
    S = tq @ tc.T
    if logq is not None:
        S = S - torch.tensor(np.asarray(logq, np.float64))[None, :]
    B = S.shape[0]
    if ids is not None:
        i = torch.tensor(np.asarray(ids).astype(np.int64))
        hit = (i[:, None] == i[None, :]) & ~torch.eye(B, dtype=torch.bool)
        S = S.masked_fill(hit, float("-inf"))
    lse = torch.logsumexp(S, 1)
    row_loss = lse - torch.diagonal(S)
    tw = torch.ones(B, dtype=torch.float64) if w is None else torch.tensor(np.asarray(w, np.float64))
    loss = (tw * row_loss).sum()
    loss.backward()
    return {"loss": float(loss.detach()), "row_loss": row_loss.detach().numpy(), "lse": lse.detach().numpy(),
            "dq": tq.grad.numpy(), "dc": tc.grad.numpy()}
