"""CPU restatement of the reference hot path — TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
import this module, and only as the checker / reported CPU baseline.  The
product (hm-retrieval-two-tower_amd/pkg) never imports it.

Every function restates SelvinSelbaraju/hm-retrieval-two-tower (cited as
/root/reference/<file>:<line>) on numpy / plain C.  The reference itself
cannot run here (TensorFlow is not installed), so parity is
pinned by the golden values of the reference's own tests
(tests/golden/reference_tests.json, checked by tests/test_oracle.py) and,
for the paths no reference test covers (gather, dedup + Adagrad, in-batch
loss and gradients, top-k tie breaking), by this restatement alone
("parity unpinned by the reference").
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from ctypes import POINTER, c_float, c_int, c_int32, c_int64, c_void_p
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "libtt_oracle.so")
_lib = None

# Keras legacy Adagrad defaults (tf.keras.optimizers.legacy.Adagrad).
ADAGRAD_INITIAL_ACCUMULATOR = 0.1
ADAGRAD_EPSILON = 1e-7
# GPU summation block (csrc/tt_sparse.hip kBlock).
GPU_DEDUP_CHUNK = 32


def build() -> str:
    """Compile the C restatement (make -C oracle) if needed; returns the .so path."""
    if not os.path.exists(_SO):
        subprocess.run(["make", "-s", "-C", _HERE], check=True)
    return _SO


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_SO)
        L.oracle_bruteforce_topk.restype = c_int
        L.oracle_bruteforce_topk.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int, c_int,
                                             c_void_p, c_void_p, c_int]
        L.oracle_scores.restype = None
        L.oracle_scores.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p]
        L.oracle_dedup_sum.restype = c_int
        L.oracle_dedup_sum.argtypes = [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]
        L.oracle_sparse_adagrad_apply.restype = None
        L.oracle_sparse_adagrad_apply.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_float,
                                                  c_float]
        _lib = L
    return _lib


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


# ---------------------------------------------------------------------------
# a1: vocab / StringLookup (features.py:106-127, input_layer.py:33-36)
def vocab_from_values(values: Sequence, max_vocab_size: Optional[int] = None) -> np.ndarray:
    """value_counts() order (count desc, first-seen on ties), head(max), str()."""
    import pandas as pd

    vc = pd.Series(list(values)).value_counts()
    idx = list(vc.head(max_vocab_size).index) if max_vocab_size else list(vc.index)
    return np.array([str(x) for x in idx])


def string_lookup(vocab: Sequence[str], values: Sequence) -> np.ndarray:
    """StringLookup(num_oov_indices=1): vocab[i] -> i+1, anything else -> 0."""
    table = {v: i + 1 for i, v in enumerate(vocab)}
    return np.array([table.get(str(v) if not isinstance(v, bytes) else v.decode(), 0) for v in values],
                    dtype=np.int32)


# ---------------------------------------------------------------------------
# a2: InputLayer.call (input_layer.py:45-69)
def gather_concat(numeric: Sequence[np.ndarray], tables: Sequence[np.ndarray], ids: Sequence[np.ndarray]) -> np.ndarray:
    """Numeric columns first, then table[ids] per categorical feature, concat."""
    cols: List[np.ndarray] = [np.asarray(v, np.float32).reshape(-1, 1) for v in numeric]
    for t, i in zip(tables, ids):
        i = np.asarray(i, np.int64).reshape(-1)
        valid = (i >= 0) & (i < t.shape[0])
        g = np.zeros((i.size, t.shape[1]), np.float32)
        g[valid] = t[i[valid]]
        cols.append(g)
    return np.concatenate(cols, axis=1) if cols else np.zeros((0, 0), np.float32)


# ---------------------------------------------------------------------------
# a7: LogQCorrection (logq_correction.py:32-42, 66-71); prob table etl/runner.py:75-78
def logq_from_lookup(candidate_ids: Sequence, lookup: Dict[str, float]) -> np.ndarray:
    """log(p[id]) in fp32 with the StaticHashTable default 1.0 (-> 0)."""
    p = np.array([lookup.get(str(x) if not isinstance(x, bytes) else x.decode(), 1.0) for x in candidate_ids],
                 dtype=np.float32)
    return np.log(p).astype(np.float32)


def logq_correction(logits: np.ndarray, candidate_ids: Sequence, lookup: Dict[str, float]) -> np.ndarray:
    """logits [B,B] - log p[candidate_ids]^T broadcast over rows."""
    return (np.asarray(logits, np.float32) - logq_from_lookup(candidate_ids, lookup)[None, :]).astype(np.float32)


def prob_lookup_from_values(values: Sequence) -> Dict[str, float]:
    """etl/runner.py:75-78: p = value_counts / len(train), keys str(id)."""
    import pandas as pd

    s = pd.Series(list(values))
    probs = s.value_counts() / len(s)
    return {str(probs.index[i]): float(probs.iloc[i]) for i in range(len(probs))}


# ---------------------------------------------------------------------------
# a5: Tower.call (tower.py:41-49, 51-75): Dense(relu)* then Dense(E, relu)
def tower_forward(x: np.ndarray, layers: Sequence[Tuple[np.ndarray, np.ndarray]], dtype=np.float64) -> np.ndarray:
    h = np.asarray(x, dtype)
    for w, b in layers:
        h = np.maximum(h @ np.asarray(w, dtype) + np.asarray(b, dtype), 0)
    return h


# ---------------------------------------------------------------------------
# a6-a8: scores, logQ, CE(from_logits, SUM) with eye labels and its gradient
# (two_tower_model.py:92, 113-124; runner.py:78-83)
def inbatch_softmax_xent(q: np.ndarray, c: np.ndarray, logq: Optional[np.ndarray] = None, pos_offset: int = 0,
                         dtype=np.float64):
    """Returns dict(loss, row_loss, lse, dq, dc) for local rows q [R,E] against
    columns c [C,E]; the positive of row i is column i + pos_offset.  dc is
    the column gradient of THIS row block (sum over blocks = full dc)."""
    q = np.asarray(q, dtype)
    c = np.asarray(c, dtype)
    R = q.shape[0]
    S = q @ c.T
    if logq is not None:
        S = S - np.asarray(logq, dtype)[None, :]
    m = S.max(axis=1)
    e = np.exp(S - m[:, None])
    lse = m + np.log(e.sum(axis=1))
    rows = np.arange(R)
    pos = rows + pos_offset
    row_loss = lse - S[rows, pos]
    P = e / e.sum(axis=1, keepdims=True)
    P[rows, pos] -= 1.0
    return {
        "loss": row_loss.sum(),
        "row_loss": row_loss,
        "lse": lse,
        "dq": P @ c,
        "dc": P.T @ q,
    }


def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 -> fp32, round to nearest even (v_cvt_pk_bf16_f32; the
    in-batch prep and P packing of csrc/tt_inbatch.hip)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


# fp32 exp / sum / log of the online softmax: |d lse| <= SOFTMAX_SLACK (1 + |lse|)
# (the slack the lse checks of tests/test_kernels_gpu.py always allowed)
SOFTMAX_SLACK = 1e-5

# log2(e) as the kernels hold it (an fp32 constant)
LOG2E_F32 = float(np.float32(1.4426950408889634))


def _exp2_arg(s32: np.ndarray, m: np.ndarray) -> np.ndarray:
    """fp32 fmaf(s, LOG2E_F32, -m) for fp32 s and integer-valued m: the fp64
    product of two fp32 values is exact and so is subtracting the integer,
    so one rounding to fp32 gives exactly the fused result."""
    return (np.asarray(s32, np.float32).astype(np.float64) * LOG2E_F32 - m).astype(np.float32)


def _softplus(x: np.ndarray) -> np.ndarray:
    return np.where(x > 0, x + np.log1p(np.exp(-np.abs(x))), np.log1p(np.exp(np.minimum(x, 0.0))))


def _not_negative(r0: int, r1: int, C: int, pos_offset: int, row_ids, col_ids) -> np.ndarray:
    """bool [r1 - r0, C]: the columns that are NO negative of rows r0 .. r1 - 1 —
    each row's positive (column i + pos_offset) and, with ids, every column
    carrying the row's id (an accidental hit)."""
    rr = np.arange(r0, r1)
    if row_ids is None:
        ex = np.zeros((r1 - r0, C), bool)
    else:
        ex = np.asarray(row_ids)[r0:r1, None] == np.asarray(col_ids)[None, :]
    ex[rr - r0, rr + pos_offset] = True
    return ex


def inbatch_softmax_xent_bf16(q: np.ndarray, c: np.ndarray, logq: Optional[np.ndarray] = None, pos_offset: int = 0,
                              rows_q: Optional[np.ndarray] = None, block: int = 2048,
                              row_ids: Optional[np.ndarray] = None, col_ids: Optional[np.ndarray] = None,
                              aux: bool = False) -> Dict[str, np.ndarray]:
    """The arithmetic contract of tt_inbatch_* (include/tt.h), restated: the
    same loss and gradients as inbatch_softmax_xent (two_tower_model.py:92,
    113-124; logq_correction.py:66-71), computed the way the kernels compute
    them, so the GPU can be held to it tightly:
      * negative pairs: S = bf16(q) . bf16(c) (RNE, exact products, rounded to
        fp32) - logq; p = fp32(2^(S log2e - M)) with M an integer (the kernel's
        running max is an integer in log2 units, so any integer gives the same
        bf16(p) up to rare last-bit ties of the fp32 exponent argument); the
        P.C product uses bf16(p) and bf16(c); the row sum L uses the fp32 p;
      * the positive pair is scored in fp32: a = lse over the negatives,
        row_loss = softplus(a - pos), dq = sigmoid(a - pos) (O / L - c_pos);
      * columns (every row i of q against c, with the rows' lse and loss):
        p = bf16(fp32(exp(bf16(q_i).bf16(c_j) - lse_i))) for the negatives,
        dc_j = exp(-logq_j) sum_i p bf16(q_i) - (-expm1(-row_loss_pos)) q_pos.
    Rows q [R,E] against columns c [C,E]; the positive of row i is column
    i + pos_offset.  `rows_q` ([C + ...] rows for the column pass; default q
    with R == C) is every row of the batch when q holds one rank's block.
    row_ids [R] / col_ids [C] (both or neither): the accidental-hit forms
    (tt_inbatch_*_hits) — a pair (i, j != pos(i)) of equal id scores -inf in
    both passes, as the kernels' accumulators start at -inf there.
    Returns dict(loss, row_loss, lse, dq) and, when the rows cover every
    column's positive (rows_q None and R == C, pos_offset 0), dc.
    aux: also the terms of the per-element contract bounds
    (inbatch_contract_bounds): sigma, g, n [R], dq_bound [R,E] and, with dc,
    dc_bound [C,E]."""
    q32, c32 = np.asarray(q, np.float32), np.asarray(c, np.float32)
    R, E = q32.shape
    C = c32.shape[0]
    qb = bf16_round(q32).astype(np.float64)
    cb = bf16_round(c32).astype(np.float64)
    lq = np.zeros(C) if logq is None else np.asarray(logq, np.float32).astype(np.float64)
    pos = np.arange(R) + pos_offset
    # fp32 positive logits (q_i . c_pos in fp64, rounded; the GPU's fp32 fma
    # chain agrees to a few ulp)
    pos_logit = (np.einsum("ij,ij->i", q32.astype(np.float64), c32[pos].astype(np.float64)) - lq[pos])
    pos_logit = pos_logit.astype(np.float32).astype(np.float64)
    row_loss = np.empty(R)
    lse = np.empty(R)
    dq = np.empty((R, E))
    g_all, n_all, A_all = np.empty(R), np.empty(R), np.empty((R, E) if aux else (0, E))
    for r0 in range(0, R, block):
        r1 = min(R, r0 + block)
        S = ((qb[r0:r1] @ cb.T) - lq[None, :]).astype(np.float32).astype(np.float64)
        ex = _not_negative(r0, r1, C, pos_offset, row_ids, col_ids)
        S[ex] = -np.inf
        mx = (S.max(axis=1) * LOG2E_F32)
        M = np.where(np.isfinite(mx), np.ceil(mx), 0.0)
        p = np.exp2(_exp2_arg(S, M[:, None]).astype(np.float64)).astype(np.float32)
        L = p.astype(np.float64).sum(axis=1)
        O = bf16_round(p).astype(np.float64) @ cb
        none = ~(L > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.where(none, -np.inf, M * np.log(2.0) + np.log(np.where(none, 1.0, L)))
            d = a - pos_logit[r0:r1]
            loss = np.where(none, 0.0, _softplus(np.where(none, 0.0, d)))
            g = np.where(none, 0.0, 1.0 / (1.0 + np.exp(-np.where(none, 0.0, d))))
            mean = np.where(none[:, None], 0.0, O / np.where(none, 1.0, L)[:, None])
        dq[r0:r1] = g[:, None] * (mean - c32[pos[r0:r1]].astype(np.float64))
        g_all[r0:r1], n_all[r0:r1] = g, (~ex).sum(axis=1)
        if aux:  # A~ = sum_j (p_ij / L_i) |bf16(c_j)|
            A_all[r0:r1] = np.where(none[:, None], 0.0,
                                    (p.astype(np.float64) @ np.abs(cb)) / np.where(none, 1.0, L)[:, None])
        row_loss[r0:r1] = loss
        lse[r0:r1] = pos_logit[r0:r1] + loss
    row_loss32 = row_loss.astype(np.float32)
    lse32 = (pos_logit.astype(np.float32) + row_loss32).astype(np.float32)
    out = {"loss": float(row_loss32.astype(np.float64).sum()), "row_loss": row_loss32, "lse": lse32,
           "dq": dq.astype(np.float32)}
    if aux:
        sigma = SOFTMAX_SLACK * (1.0 + np.abs(lse32.astype(np.float64)))
        out.update(sigma=sigma, g=g_all, n=n_all)
        out["dq_bound"] = (g_all * (2.0 ** -7 + 2.0 * sigma + n_all * 2.0 ** -24))[:, None] * A_all \
            + (np.expm1(sigma) + 2.0 ** -21)[:, None] * np.abs(dq) \
            + FP32_TINY * (1.0 + A_all + np.abs(c32[pos].astype(np.float64)) + (n_all * np.abs(cb).max())[:, None])
    if rows_q is None and R == C and pos_offset == 0:
        dc = inbatch_cols_bf16(q32, lse32, row_loss32, c32, logq, 0, block, row_ids, col_ids, aux)
        if aux:
            dc, out["dc_bound"] = dc
        out["dc"] = dc
    return out


def inbatch_cols_bf16(q_all: np.ndarray, lse: np.ndarray, row_loss: np.ndarray, c: np.ndarray,
                      logq: Optional[np.ndarray] = None, pos_offset: int = 0, block: int = 2048,
                      row_ids: Optional[np.ndarray] = None, col_ids: Optional[np.ndarray] = None, aux: bool = False):
    """Column pass of the contract (inbatch_softmax_xent_bf16): dc [C,E] of the
    columns c against every row q_all [R,E] with its lse and row_loss; the
    positive of column j is row j + pos_offset.  row_ids [R] / col_ids [C]:
    pairs of equal id other than the positive at -inf (the hits forms).
    aux: returns (dc, dc_bound), the per-element bound of
    inbatch_contract_bounds."""
    q32, c32 = np.asarray(q_all, np.float32), np.asarray(c, np.float32)
    R, E = q32.shape
    C = c32.shape[0]
    qb = bf16_round(q32).astype(np.float64)
    cb = bf16_round(c32).astype(np.float64)
    lse64 = np.asarray(lse, np.float32).astype(np.float64)
    O = np.zeros((C, E))
    Ob = np.zeros((C, E))
    cols = np.arange(C)
    sigma = SOFTMAX_SLACK * (1.0 + np.abs(lse64))
    for r0 in range(0, R, block):
        r1 = min(R, r0 + block)
        s = ((qb[r0:r1] @ cb.T) - lse64[r0:r1, None]).astype(np.float32).astype(np.float64)
        hit = (cols + pos_offset >= r0) & (cols + pos_offset < r1)
        s[cols[hit] + pos_offset - r0, cols[hit]] = -np.inf
        if row_ids is not None:
            s[np.asarray(row_ids)[r0:r1, None] == np.asarray(col_ids)[None, :]] = -np.inf
        p = np.exp2(_exp2_arg(s, 0.0).astype(np.float64)).astype(np.float32)
        O += bf16_round(p).astype(np.float64).T @ qb[r0:r1]
        if aux:
            w = 2.0 ** -7 + 2.0 * sigma[r0:r1] + R * 2.0 ** -24
            Ob += p.astype(np.float64).T @ (w[:, None] * np.abs(qb[r0:r1]))
    scale = np.ones(C) if logq is None else np.exp(-np.asarray(logq, np.float32).astype(np.float64))
    omp = -np.expm1(-np.asarray(row_loss, np.float32).astype(np.float64)[cols + pos_offset])
    dc = O * scale[:, None] - omp[:, None] * q32[cols + pos_offset].astype(np.float64)
    if not aux:
        return dc.astype(np.float32)
    bound = Ob * scale[:, None] + (omp * np.expm1(sigma[cols + pos_offset]))[:, None] \
        * np.abs(q32[cols + pos_offset].astype(np.float64)) + 2.0 ** -21 * np.abs(dc) \
        + FP32_TINY * (1.0 + np.abs(q32.astype(np.float64)).sum(axis=0))[None, :]
    return dc.astype(np.float32), bound


# bf16 operands (8 significant bits, round to nearest): unit roundoff 2^-8 per
# operand, so a product of two rounded operands is within 2^-7 + 2^-16 of the
# exact one; fp32 accumulation of <= 128 exact bf16 products adds < 2^-17.
BF16_DOT_EPS = 2.0 ** -7 + 2.0 ** -15


def inbatch_error_bound(q: np.ndarray, c: np.ndarray, pos_offset: int = 0) -> Dict[str, np.ndarray]:
    """Certified bound of the fused bf16-MFMA loss against the exact one.

    Each score S'_ij is computed from bf16(q_i) . bf16(c_j):
      |S~_ij - S_ij| <= d_ij = BF16_DOT_EPS * sum_k |q_ik| |c_jk|.
    lse is a softmax-weighted mean of the perturbations, so
      |lse~_i - lse_i| <= max_j d_ij  (+ fp32 softmax arithmetic, ~1e-5 |lse|),
    and the positive logit is an fp32 dot product, so the row loss has the
    same bound and the batch loss at most the sum of the rows'.
    Returns dict(lse=[R], loss=float)."""
    A = np.abs(np.asarray(q, np.float64)) @ np.abs(np.asarray(c, np.float64)).T
    row = BF16_DOT_EPS * A.max(axis=1)
    return {"lse": row, "loss": float(row.sum())}


# ---------------------------------------------------------------------------
# Per-element checks of the in-batch loss (DESIGN.md §6 "Per-element
# guarantees"): a cancellation-free fp64 reference, certified bounds of the
# kernels' error against it, and the contract's own per-element residual.
def _sigmoid(x: np.ndarray) -> np.ndarray:
    """exp(-softplus(-x)): keeps full relative accuracy where sigmoid(x) ~ e^x."""
    return np.exp(-_softplus(-x))


def inbatch_reference(q: np.ndarray, c: np.ndarray, logq: Optional[np.ndarray] = None, pos_offset: int = 0,
                      row_ids: Optional[np.ndarray] = None, col_ids: Optional[np.ndarray] = None,
                      rows_q: Optional[np.ndarray] = None, block: int = 1024) -> Dict[str, np.ndarray]:
    """The loss of inbatch_softmax_xent in fp64 WITHOUT its cancellations
    (lse - S_pos is exactly 0.0 once the positive outweighs the negatives by
    2^53; softmax - I loses the same digits), in the form the kernels use.
    Rows q [R,E] against columns c [C,E]; the positive of row i is column
    i + pos_offset; N_i = every other column, less (with ids) those carrying
    row i's id.  Over the negatives j in N_i:
      s_ij = q_i . c_j - logq_j,  a_i = logsumexp_j s_ij,  w_ij = exp(s_ij - a_i)
      d_i = a_i - pos_i,  row_loss_i = softplus(d_i),  g_i = sigmoid(d_i) = 1 - P_pos
      lse_i = logaddexp(a_i, pos_i)
      mean_i = sum_j w_ij c_j,  A_i = sum_j w_ij |c_j|,  dq_i = g_i (mean_i - c_pos)
      P_ij = exp(s_ij - lse_i) = g_i w_ij,  dc_j = sum_i P_ij q_i - g_pos(j) q_pos(j)
    and where N_i is empty everything is 0 (lse_i = pos_i), as the kernels do.
    dc is the column gradient of THIS row block; rows_q (every row of the
    batch, q being its rows pos_offset .. pos_offset + R - 1, the rows' ids
    being col_ids[:len(rows_q)]): dc of the whole batch instead.
    Returns dict(loss, row_loss, lse, dq, dc) and the bounds' intermediates
    (a, pos, d, g, n, mean, A [R,E], cpos [R,E]) and arguments (logq,
    pos_offset, row_ids, col_ids)."""
    if rows_q is not None:
        ids_all = None if col_ids is None else np.asarray(col_ids)[:len(rows_q)]
        full = inbatch_reference(rows_q, c, logq, 0, ids_all, col_ids, None, block)
        sl = slice(pos_offset, pos_offset + len(q))
        out = {k: (v[sl] if k not in ("dc", "logq", "col_ids") and isinstance(v, np.ndarray) else v)
               for k, v in full.items()}
        out["loss"] = float(out["row_loss"].sum())
        out["pos_offset"] = pos_offset
        return out
    q, c = np.asarray(q, np.float64), np.asarray(c, np.float64)
    R, E = q.shape
    C = c.shape[0]
    lq = np.zeros(C) if logq is None else np.asarray(logq, np.float64)
    out = {k: np.zeros(R) for k in ("row_loss", "lse", "a", "pos", "d", "g", "n")}
    out.update({k: np.zeros((R, E)) for k in ("dq", "mean", "A", "cpos")})
    dc = np.zeros((C, E))
    for r0 in range(0, R, block):
        r1 = min(R, r0 + block)
        b = slice(r0, r1)
        rr = np.arange(r0, r1)
        S = q[b] @ c.T - lq[None, :]
        pos = S[rr - r0, rr + pos_offset].copy()
        ex = _not_negative(r0, r1, C, pos_offset, row_ids, col_ids)
        S[ex] = -np.inf
        mx = S.max(axis=1)
        none = ~np.isfinite(mx)
        mx = np.where(none, 0.0, mx)
        e = np.exp(S - mx[:, None])
        L = e.sum(axis=1)
        with np.errstate(divide="ignore"):
            a = np.where(none, -np.inf, mx + np.log(np.where(none, 1.0, L)))
        w = e / np.where(none, 1.0, L)[:, None]
        d = np.where(none, -np.inf, a - pos)
        dz = np.where(none, 0.0, d)
        g = np.where(none, 0.0, _sigmoid(dz))
        cpos = c[rr + pos_offset]
        out["row_loss"][b] = np.where(none, 0.0, _softplus(dz))
        out["lse"][b] = np.where(none, pos, np.logaddexp(np.where(none, pos, a), pos))
        out["a"][b], out["pos"][b], out["d"][b], out["g"][b], out["n"][b] = a, pos, d, g, (~ex).sum(axis=1)
        out["mean"][b], out["A"][b], out["cpos"][b] = w @ c, w @ np.abs(c), cpos
        out["dq"][b] = g[:, None] * (out["mean"][b] - cpos)
        dc += (w * g[:, None]).T @ q[b]
        dc[rr + pos_offset] -= g[:, None] * q[b]
    out.update(dc=dc, loss=float(out["row_loss"].sum()), logq=None if logq is None else lq, pos_offset=pos_offset,
               row_ids=row_ids, col_ids=col_ids)
    return out


# x3 forms: bf16x3 products hi.hi + hi.lo + lo.hi of operands split x = hi +
# lo + r, hi = bf16(x), lo = bf16(x - hi).  bf16 keeps 8 significant bits, so
# round to nearest gives |x - hi| <= 2^-8 |x| in the worst case (x just above
# a power of two; 2^-9 just below one) and |r| <= 2^-8 |x - hi| <= 2^-16 |x|.
# Per product x y, relative to |x||y|:
#   the dropped lo.lo term             |lo_x lo_y|  <= 2^-16
#   each operand's rounded-off residual |r_x y|, |x r_y|  <= 2^-16 each
#   the fp32 accumulation of the 3 E / 16 <= 24 MFMA results of a score
#     (2^-24 each, against sum_k |x_k||y_k|; the bias's share is in sigma)  < 2^-19
# so eps = 3 2^-16 + 2^-19 = 25 2^-19.  (Each of the three 2^-16 terms is 2^-18
# when the operands sit mid-binade, which gives the 2^-16 often quoted for
# bf16x3; the certified value takes the worst case.)  P is split hi / lo in
# registers in the same way and multiplied with the split c (or q) by the
# same three products: 3 2^-16 per term, taken by inbatch_bounds as (1 + u)^2
# - 1 >= 2 u with u = 3 2^-17 (the P.V accumulation is its n 2^-24 term).
X3_DOT_EPS = 25 * 2.0 ** -19
X3_P_U = 3 * 2.0 ** -17
# bf16 forms: eps = BF16_DOT_EPS, u = 2^-8 (bf16(p) and the bf16 operand of P.V)
BF16_P_U = 2.0 ** -8
# rows whose weight error alpha reaches this are not certified against fp64
ALPHA_CAP = 0.25
# the smallest normal fp32: g, a weight p or an output below it may be flushed to 0
FP32_TINY = 2.0 ** -126


def inbatch_bounds(ref: Dict[str, np.ndarray], q: np.ndarray, c: np.ndarray, eps: float, u: float,
                   n_rows_total: Optional[int] = None, block: int = 1024) -> Dict[str, np.ndarray]:
    """Certified per-element bounds of a kernel's lse, row_loss, dq and dc
    against inbatch_reference (`ref`, of the same q, c), for a kernel whose
    negative scores carry a relative product-sum error eps (|s~_ij - s_ij| <=
    D_ij = eps sum_k |q_ik||c_jk|) and whose p and second P.V operand are each
    rounded to relative u.  With n_i = |N_i|, E the embedding size and R the
    number of rows a column sums over (n_rows_total, default len(q)):
      sigma_i  = SOFTMAX_SLACK (1 + |lse_i|)      fp32 exp / sum / log
      delta_i  = max_{j in N_i} D_ij + sigma_i    bounds |a~_i - a_i| (a is a
                 softmax-weighted mean of the score perturbations)
      delta'_i = delta_i + E 2^-24 sum_k |q_ik||c_pos,k|   and the fp32 positive
      alpha_i  = e^delta_i (1 + u)^2 - 1 + n_i 2^-24       one weight of P.V
    Bounds (returned under these keys):
      lse        delta'_i + 2^-23 |lse_i|  (lse = logaddexp(a, pos) moves by
                 at most max(|da|, |dpos|); its fp32 store)
      row_loss   delta'_i, and log_row_loss = delta'_i + 2^-21 on
                 |ln loss~ - ln loss|: softplus and ln softplus are both
                 1-Lipschitz in d (d/dd ln softplus(d) = sigmoid(d) /
                 softplus(d) <= 1), the 2^-21 for fp32 expf / log1pf.  The
                 second binds on confident rows (loss << delta').
      dq         g_i e^delta'_i 2 alpha_i A_ik / (1 - alpha_i)
                 + g_i (e^delta'_i - 1) |mean_ik - c_pos,k| + 2^-21 |dq_ik|
      dc         sum_i P_ij F_ij |q_ik| + g_pos (e^delta'_pos - 1) |q_pos,k|
                 + 2^-21 |dc_jk|,  F_ij = e^(D_ij + delta_i) (1 + u)^2 - 1 + R 2^-24
    Mean term: the kernel's mean is sum_j w~_ij c~_j / sum_j w^_ij, where every
    numerator weight (its score error, bf16 / split p, rounded c_j, fp32
    accumulation) is w_ij (1 + x_ij), |x_ij| <= alpha_i, and every denominator
    weight (score error and fp32 sum only) is w_ij (1 + y_ij), |y_ij| <=
    e^delta_i - 1 <= alpha_i.  So the numerator is off by at most alpha_i A_ik,
    the denominator lies in [1 - alpha_i, 1 + alpha_i], and
      |mean~ - mean| <= (alpha A + alpha |mean|) / (1 - alpha) <= 2 alpha A / (1 - alpha)
    since |mean_ik| <= A_ik.  g and 1 - P_pos: g = sigmoid(d) and
    |d ln sigmoid(d) / dd| = 1 - sigmoid(d) <= 1, so |d~ - d| <= delta' gives
    g~ / g in [e^-delta', e^delta']: the factor e^delta' on the mean term and
    the term g (e^delta' - 1) |mean - c_pos|; the cols pass's P_ij = exp(s_ij -
    lse_i) carries e^(D_ij + delta_i) in the same way.
    fp32 range: g = 1 / (1 + expf(pos - a)), a weight p and every output may be
    flushed to 0 below FP32_TINY = 2^-126 (g from pos - a > 87.3), where no
    relative bound can hold: dq gets + FP32_TINY (1 + |mean_ik - c_pos,k| +
    n_i max|c|) and dc + FP32_TINY (1 + sum_i |q_ik|).
    The dc bound sums over the rows of `ref`: it bounds the dc of that row
    block (of the whole batch when ref holds every row, not a rows_q block).
    Rows with alpha_i >= ALPHA_CAP are not certified (`certified` [R], `alpha`
    [R]); their dq bound is +inf.  Also returned: delta, delta_pos (delta') and
    dc_pos, the g_pos term of the dc bound on its own (the cols entry without
    row_loss takes 1 - P_pos from -expm1(pos - lse) and meets a wider one)."""
    q64, c64 = np.asarray(q, np.float64), np.asarray(c, np.float64)
    R, E = q64.shape
    C = c64.shape[0]
    Rt = R if n_rows_total is None else n_rows_total
    off, row_ids, col_ids = ref["pos_offset"], ref["row_ids"], ref["col_ids"]
    lq = np.zeros(C) if ref["logq"] is None else ref["logq"]
    aq, ac = np.abs(q64), np.abs(c64)
    sigma = SOFTMAX_SLACK * (1.0 + np.abs(ref["lse"]))
    delta, delta_p = np.empty(R), np.empty(R)
    dc_b, dc_pos = np.zeros((C, E)), np.zeros((C, E))
    for r0 in range(0, R, block):
        r1 = min(R, r0 + block)
        b = slice(r0, r1)
        rr = np.arange(r0, r1)
        D = eps * (aq[b] @ ac.T)
        ex = _not_negative(r0, r1, C, off, row_ids, col_ids)
        delta[b] = np.where(ex, 0.0, D).max(axis=1) + sigma[b]
        delta_p[b] = delta[b] + E * 2.0 ** -24 * D[rr - r0, rr + off] / eps
        with np.errstate(over="ignore"):
            P = np.exp(q64[b] @ c64.T - lq[None, :] - ref["lse"][b, None])
        P[ex] = 0.0
        F = np.exp(D + delta[b, None]) * (1.0 + u) ** 2 - 1.0 + Rt * 2.0 ** -24
        dc_b += (P * F).T @ aq[b]
        dc_pos[rr + off] += (ref["g"][b] * np.expm1(delta_p[b]))[:, None] * aq[b]
    dc_b += dc_pos + 2.0 ** -21 * np.abs(ref["dc"]) + FP32_TINY * (1.0 + aq.sum(axis=0))[None, :]
    alpha = np.exp(delta) * (1.0 + u) ** 2 - 1.0 + ref["n"] * 2.0 ** -24
    cert = alpha < ALPHA_CAP
    al = np.where(cert, alpha, 0.0)
    g = ref["g"]
    dq_b = (g * np.exp(delta_p) * 2.0 * al / (1.0 - al))[:, None] * ref["A"] \
        + (g * np.expm1(delta_p))[:, None] * np.abs(ref["mean"] - ref["cpos"]) + 2.0 ** -21 * np.abs(ref["dq"]) \
        + FP32_TINY * (1.0 + np.abs(ref["mean"] - ref["cpos"]) + (ref["n"] * ac.max())[:, None])
    dq_b[~cert] = np.inf
    return {"lse": delta_p + 2.0 ** -23 * np.abs(ref["lse"]), "row_loss": delta_p,
            "log_row_loss": delta_p + 2.0 ** -21,
            "dq": dq_b, "dc": dc_b, "dc_pos": dc_pos, "alpha": alpha, "certified": cert, "delta": delta,
            "delta_pos": delta_p}


def inbatch_contract_bounds(con: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """Per-element bounds of the bf16 kernels against their contract
    restatement `con` = inbatch_softmax_xent_bf16(..., aux=True), for the
    regimes where inbatch_bounds certifies nothing about bf16 scores (wide
    score spreads: alpha >= ALPHA_CAP; the x3 forms exist for those).  With
    sigma_i = SOFTMAX_SLACK (1 + |lse_i|), A~ and P~ from the restatement's
    own bf16 scores:
      lse       sigma_i
      row_loss  sigma_i, and log_row_loss = sigma_i + 2^-21 (as inbatch_bounds)
      dq        g_i (2^-7 + 2 sigma_i + n_i 2^-24) A~_ik + (e^sigma_i - 1 + 2^-21) |dq_ik|
      dc        sum_i P~_ij (2^-7 + 2 sigma_i + R 2^-24) |bf16(q_ik)| exp(-logq_j)
                + g_pos (e^sigma_pos - 1) |q_pos,k| + 2^-21 |dc_jk|
    The 2^-7 is the contract's stated residual: fp32 summation order and the
    last bit of the exp argument can each move a bf16(p) by at most one bf16
    ulp (<= 2^-7 relative); 2 sigma covers p's numerator and L; the rest is
    the fp32 accumulation and g as in inbatch_bounds, and so is the fp32 range
    term FP32_TINY (...) of dq and dc.  Derived, not observed."""
    out = {"lse": con["sigma"], "row_loss": con["sigma"], "log_row_loss": con["sigma"] + 2.0 ** -21,
           "dq": con["dq_bound"], "certified": np.ones(len(con["sigma"]), bool)}
    if "dc_bound" in con:
        out["dc"] = con["dc_bound"]
    return out


# ---------------------------------------------------------------------------
# a3/a4: dedup + sparse Adagrad (legacy Keras optimizer; see tt_oracle.c)
def dedup_sum(ids: np.ndarray, grad: np.ndarray, chunk: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    ids = _i32(ids).reshape(-1)
    grad = _f32(grad)
    n, dim = grad.shape
    uniq = np.empty(max(n, 1), np.int32)
    sums = np.empty((max(n, 1), dim), np.float32)
    u = lib().oracle_dedup_sum(ids.ctypes.data, n, grad.ctypes.data, grad.strides[0] // 4, dim, chunk,
                               uniq.ctypes.data, sums.ctypes.data)
    return uniq[:u].copy(), sums[:u].copy()


def sparse_adagrad(table: np.ndarray, accum: np.ndarray, ids: np.ndarray, grad: np.ndarray, lr: float,
                   eps: float = ADAGRAD_EPSILON, chunk: int = GPU_DEDUP_CHUNK) -> None:
    """In place: dedup (ids out of [0, rows) skipped) then Adagrad per distinct row."""
    ids = _i32(ids).reshape(-1)
    valid = (ids >= 0) & (ids < table.shape[0])
    uniq, sums = dedup_sum(ids[valid], _f32(grad)[valid], chunk)
    assert table.dtype == np.float32 and accum.dtype == np.float32 and table.flags.c_contiguous
    lib().oracle_sparse_adagrad_apply(table.ctypes.data, accum.ctypes.data, table.shape[1], uniq.ctypes.data,
                                      sums.ctypes.data, len(uniq), lr, eps)


def dense_adagrad(param: np.ndarray, accum: np.ndarray, grad: np.ndarray, lr: float,
                  eps: float = ADAGRAD_EPSILON) -> None:
    """ResourceApplyAdagradV2: accum += g^2; var -= g*lr / (sqrt(accum) + eps) (fp32, in place)."""
    g = _f32(grad)
    lr = np.float32(lr)
    eps = np.float32(eps)
    accum += g * g
    param -= (g * lr) / (np.sqrt(accum) + eps)


def adam_powers(beta1, beta2, step) -> Tuple[np.float32, np.float32]:
    """(beta1^step, beta2^step) as the fp32 optimizers compute them (powf)."""
    f = np.float32
    return f(np.power(f(beta1), f(step))), f(np.power(f(beta2), f(step)))


def dense_adam(param, m, v, grad, lr, beta1, beta2, eps, step) -> None:
    """ResourceApplyAdam (fp32, in place)."""
    f = np.float32
    g = _f32(grad)
    b1p, b2p = adam_powers(beta1, beta2, step)
    alpha = f((f(lr) * np.sqrt(f(1) - b2p)) / (f(1) - b1p))
    m += (g - m) * (f(1) - f(beta1))
    v += (g * g - v) * (f(1) - f(beta2))
    param -= (m * alpha) / (np.sqrt(v) + f(eps))


def sparse_adam(table, m, v, ids, grad, lr, beta1, beta2, eps, step, chunk: int = GPU_DEDUP_CHUNK) -> None:
    """Legacy Adam._resource_apply_sparse after dedup (fp32, in place)."""
    f = np.float32
    ids = _i32(ids).reshape(-1)
    valid = (ids >= 0) & (ids < table.shape[0])
    uniq, sums = dedup_sum(ids[valid], _f32(grad)[valid], chunk)
    b1p, b2p = adam_powers(beta1, beta2, step)
    lr_t = f(f(lr) * (np.sqrt(f(1) - b2p) / (f(1) - b1p)))
    m *= f(beta1)
    v *= f(beta2)
    m[uniq] += sums * (f(1) - f(beta1))
    v[uniq] += (sums * sums) * (f(1) - f(beta2))
    table -= (lr_t * m) / (np.sqrt(v) + f(eps))


# ---------------------------------------------------------------------------
# a10: BruteForceIndex.call (brute_force.py:75-83)
def bruteforce_topk(q: np.ndarray, c: np.ndarray, k: int, threads: int = 0) -> Tuple[np.ndarray, np.ndarray, int]:
    """Exact fp32 fmaf-chain scores, top-k (score desc, index asc).  Returns
    (scores [Q,k], indices [Q,k] int32, threads used)."""
    q = _f32(q)
    c = _f32(c)
    nq, d = q.shape
    n = c.shape[0]
    if k > n:
        raise ValueError(f"k={k} > number of candidates {n}")
    out_s = np.empty((nq, k), np.float32)
    out_i = np.empty((nq, k), np.int32)
    used = lib().oracle_bruteforce_topk(q.ctypes.data, d, nq, c.ctypes.data, d, n, d, k, out_s.ctypes.data,
                                        out_i.ctypes.data, threads)
    return out_s, out_i, used


def fmaf_scores(q: np.ndarray, c: np.ndarray) -> np.ndarray:
    q = _f32(q)
    c = _f32(c)
    out = np.empty((q.shape[0], c.shape[0]), np.float32)
    lib().oracle_scores(q.ctypes.data, q.shape[1], q.shape[0], c.ctypes.data, c.shape[1], c.shape[0], q.shape[1],
                        out.ctypes.data)
    return out


def topk_merge(scores: np.ndarray, idx: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """[L,Q,k_in] sorted lists -> global top-k with the top_k order."""
    L, Q, kin = scores.shape
    s = np.transpose(scores, (1, 0, 2)).reshape(Q, L * kin)
    i = np.transpose(idx, (1, 0, 2)).reshape(Q, L * kin)
    order = np.lexsort((i, -s.astype(np.float64)), axis=1)[:, :k]
    return np.take_along_axis(s, order, 1), np.take_along_axis(i, order, 1)


# ---------------------------------------------------------------------------
# StaticIndex.call (static_index.py:37-55) and IndexRecall (index_recall.py:22-59)
def static_index(candidates: Sequence, k: int, batch: int) -> np.ndarray:
    row = np.asarray(list(candidates)[:k])
    return np.tile(row[None, :], (batch, 1))


class RecallAccumulator:
    """hits[k] += sum(equal(true, cands[:, :k])) (int32); metric = hits/seen (float64)."""

    def __init__(self, ks: Sequence[int]):
        self.ks = list(ks)
        self.hits = {k: 0 for k in self.ks}
        self.seen = 0
        self.metric: Dict[int, float] = {}

    def update(self, true_ids: Sequence, candidates: np.ndarray) -> Dict[int, float]:
        t = np.asarray(list(true_ids)).reshape(-1, 1)
        self.seen += t.shape[0]
        for k in self.ks:
            self.hits[k] += int(np.sum(t == candidates[:, :k]))
            self.metric[k] = np.float64(self.hits[k]) / np.float64(self.seen)
        return self.metric


# ---------------------------------------------------------------------------
# CPU baseline: one full train step (TwoTowerModel.train_step,
# two_tower_model.py:94-130, with legacy Adagrad) in numpy fp32.
def glorot_uniform(rng: np.random.Generator, fan_in: int, fan_out: int) -> np.ndarray:
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, size=(fan_in, fan_out)).astype(np.float32)


class CpuTwoTower:
    """fp32 numpy train step: gather -> towers -> scores/logQ/CE-SUM -> grads ->
    dense Adagrad (MLP) + dedup + sparse Adagrad (tables)."""

    def __init__(self, q_tables: List[np.ndarray], c_tables: List[np.ndarray], q_layers, c_layers, lr: float,
                 inbatch: str = "fp32"):
        """inbatch: "fp32" — the in-batch scores, softmax and gradients in
        fp32 (the reference's arithmetic); "bf16" — the gradients dQ, dC by
        the kernels' arithmetic contract (inbatch_softmax_xent_bf16), the
        returned loss still the fp32 one (self.last_contract_loss holds the
        contract's)."""
        if inbatch not in ("fp32", "bf16"):
            raise ValueError(f"inbatch must be 'fp32' or 'bf16', got {inbatch!r}")
        self.inbatch = inbatch
        self.last_contract_loss = None
        self.q_tables, self.c_tables = q_tables, c_tables
        self.q_layers = [[w.copy(), b.copy()] for w, b in q_layers]
        self.c_layers = [[w.copy(), b.copy()] for w, b in c_layers]
        self.lr = lr
        acc = ADAGRAD_INITIAL_ACCUMULATOR
        self.q_acc = [np.full_like(t, acc) for t in q_tables]
        self.c_acc = [np.full_like(t, acc) for t in c_tables]
        self.ql_acc = [[np.full_like(w, acc), np.full_like(b, acc)] for w, b in self.q_layers]
        self.cl_acc = [[np.full_like(w, acc), np.full_like(b, acc)] for w, b in self.c_layers]

    @staticmethod
    def _tower(x, layers):
        acts = [x]
        for w, b in layers:
            acts.append(np.maximum(acts[-1] @ w + b, 0).astype(np.float32))
        return acts

    @staticmethod
    def _tower_bwd(acts, layers, g):
        grads = []
        for li in range(len(layers) - 1, -1, -1):
            w, _ = layers[li]
            g = g * (acts[li + 1] > 0)
            grads.append((acts[li].T @ g, g.sum(0)))
            g = g @ w.T
        return grads[::-1], g

    def forward(self, q_ids: List[np.ndarray], c_ids: List[np.ndarray]):
        """Both towers' activations [x, h_1, ..., h_L] (fp32)."""
        xq = gather_concat([], self.q_tables, q_ids)
        xc = gather_concat([], self.c_tables, c_ids)
        return self._tower(xq, self.q_layers), self._tower(xc, self.c_layers)

    @staticmethod
    def _scores_loss(Q, C, logq):
        """fp32 scores - logQ, softmax terms and the CE-SUM loss
        (two_tower_model.py:92,113-122, logq_correction.py:66-71)."""
        S = Q @ C.T
        if logq is not None:
            S -= logq[None, :]
        m = S.max(1, keepdims=True)
        e = np.exp(S - m)
        z = e.sum(1, keepdims=True)
        B = S.shape[0]
        loss = float(np.sum(np.log(z[:, 0]) + m[:, 0] - S[np.arange(B), np.arange(B)]))
        return S, m, e, z, loss

    def loss_only(self, q_ids: List[np.ndarray], c_ids: List[np.ndarray], logq: Optional[np.ndarray]) -> float:
        """The fp32 loss of a batch from this restatement's own forward (no update)."""
        qa, ca = self.forward(q_ids, c_ids)
        return self._scores_loss(qa[-1], ca[-1], logq)[-1]

    def step(self, q_ids: List[np.ndarray], c_ids: List[np.ndarray], logq: Optional[np.ndarray],
             acts=None) -> float:
        """One train step.  acts: optional (query, candidate) activation lists
        to use instead of this restatement's own forward (a caller holding
        another implementation's forward — equal to this one within fp32
        rounding — checks the rest of the step against the same ReLU masks: a
        unit whose pre-activation rounds to the other side of 0 would otherwise
        switch a whole row's gradient path)."""
        if acts is None:
            qa, ca = self.forward(q_ids, c_ids)
        else:
            qa, ca = [np.asarray(a, np.float32) for a in acts[0]], [np.asarray(a, np.float32) for a in acts[1]]
        Q, C = qa[-1], ca[-1]
        S, m, e, z, loss = self._scores_loss(Q, C, logq)
        B = S.shape[0]
        if self.inbatch == "bf16":
            del S, e
            r = inbatch_softmax_xent_bf16(Q, C, logq)
            self.last_contract_loss = r["loss"]
            dQ, dC = r["dq"], r["dc"]
        else:
            P = e / z
            P[np.arange(B), np.arange(B)] -= 1.0
            dQ = P @ C
            dC = P.T @ Q
        gq, dxq = self._tower_bwd(qa, self.q_layers, dQ)
        gc, dxc = self._tower_bwd(ca, self.c_layers, dC)
        for layers, accs, grads in ((self.q_layers, self.ql_acc, gq), (self.c_layers, self.cl_acc, gc)):
            for (w, b), (aw, ab), (dw, db) in zip(layers, accs, grads):
                dense_adagrad(w, aw, dw, self.lr)
                dense_adagrad(b, ab, db, self.lr)
        # A table looked up by several features gets ONE update from the
        # concatenation of its lookups (TF aggregates the IndexedSlices of a
        # variable used twice before the sparse apply).
        for tables, accs, ids, dx in ((self.q_tables, self.q_acc, q_ids, dxq), (self.c_tables, self.c_acc, c_ids, dxc)):
            groups = {}
            off = 0
            for t, a, i in zip(tables, accs, ids):
                g = groups.setdefault(id(t), [t, a, [], []])
                g[2].append(np.asarray(i, np.int32).reshape(-1))
                g[3].append(dx[:, off:off + t.shape[1]])
                off += t.shape[1]
            for t, a, il, gl in groups.values():
                sparse_adagrad(t, a, np.concatenate(il), np.concatenate(gl), self.lr)
        return loss
