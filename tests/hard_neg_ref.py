"""fp64 reference of hard-negative mining in the in-batch loss (include/tt.h,
"hard negatives"), shared by tests/test_hard_neg_host.py and
tests/test_hard_neg_gpu.py.

  scores()      S'[i][j] = q_i . c_j - logq[j] in fp64 under one arithmetic's
                operand rounding ("bf16": bf16(q) . bf16(c); "x3": hi.hi +
                hi.lo + lo.hi of the bf16 split operands; "fp64": the fp32
                operands as they are)
  select()      a, b, thr and the kept mask of every row, by a full sort
  reference()   lse, row_loss, dq, dc over the kept set through
                inbatch_rowwise.reference_torch: a dropped pair is handed to
                it exactly as an accidental hit is (its "not a negative"
                matrix), so the per-element bounds and violations() apply
  bounds()      inbatch_rowwise.bounds_torch of the same masked problem
  exact_case()  inputs on which every product and sum is exact in fp32
  gap_case()    the small end-to-end case with a certified gap a - b

Everything here works on torch tensors of any device.
"""
import functools

import numpy as np
import torch

import inbatch_rowwise
from oracle import oracle

NINF = float("-inf")


def bf16(x):
    return x.float().bfloat16().double()


def scores(q, c, logq, form):
    """fp64 [R, C] scores under `form`'s operand rounding (logq may be None)."""
    qd, cd = q.double(), c.double()
    if form == "bf16":
        S = bf16(q) @ bf16(c).T
    elif form == "x3":
        qh, ch = bf16(q), bf16(c)
        ql, cl = bf16((qd - qh).float()), bf16((cd - ch).float())
        S = qh @ ch.T + qh @ cl.T + ql @ ch.T
    else:
        S = qd @ cd.T
    return S if logq is None else S - logq.double()[None, :]


def hit_matrix(row_ids, col_ids, R, C, dev):
    if row_ids is None:
        return torch.zeros(R, C, dtype=torch.bool, device=dev)
    return row_ids[:, None] == col_ids[None, :]


def select(S, k, pos_offset=0, row_ids=None, col_ids=None):
    """The contract's selection on fp64 scores S [R, C]: dict(a, b (fp64, nan
    where the row has no such rank), thr (fp32), kept [R, C] bool over the
    negatives (the positive's entry False), negs [R] the rows' negatives)."""
    R, C = S.shape
    dev = S.device
    rr = torch.arange(R, device=dev)
    V = S.masked_fill(hit_matrix(row_ids, col_ids, R, C, dev), NINF)  # hits stay negatives, at -inf
    pos = torch.zeros(R, C, dtype=torch.bool, device=dev)
    pos[rr, rr + pos_offset] = True
    # the positive leaves the row: sort the other C - 1 values
    W = V[~pos].view(R, C - 1) if C > 1 else V.new_zeros(R, 0)
    W = torch.sort(W, dim=1, descending=True).values
    negs = C - 1
    nan = torch.full((R,), float("nan"), dtype=torch.float64, device=dev)
    if negs <= k:
        a = W[:, k - 1].clone() if negs == k else nan
        thr = torch.full((R,), NINF, dtype=torch.float32, device=dev)
        b = nan
    else:
        a, b = W[:, k - 1].clone(), W[:, k].clone()
        mid = (0.5 * a + 0.5 * b).float()  # exact in fp64, one rounding to fp32
        thr = torch.where((a > b) & (mid.double() == b), a.float(), mid)
        thr = torch.where(torch.isinf(b) & (b < 0), torch.full_like(thr, NINF), thr)
    kept = (V >= thr.double()[:, None]) & ~pos & torch.isfinite(V)  # a hit (-inf) has weight 0 whatever thr is
    return {"a": a, "b": b, "thr": thr, "kept": kept, "negs": negs}


class _Rows:
    """Stands where reference_torch / bounds_torch take row_ids: their
    `row_ids[r0:r1, None] == col_ids[None, :]` becomes the block [r0, r1) of
    a given "not a negative" matrix."""

    def __init__(self, ex):
        self.ex = ex

    def __getitem__(self, key):
        return _Block(self.ex[key[0]])


class _Block:
    def __init__(self, ex):
        self.ex = ex

    def __eq__(self, other):
        return self.ex.clone()

    __hash__ = None


class _Cols:
    def __getitem__(self, key):
        return self


def reference(q, c, logq, kept, pos_offset=0):
    """reference_torch of the loss over the kept negatives (fp64 of the fp32
    operands; every pair outside kept and off the positive masked)."""
    return inbatch_rowwise.reference_torch(q, c, logq, pos_offset, _Rows(~kept), _Cols())


def bounds(ref, q, c, form, n_rows_total=None):
    return inbatch_rowwise.bounds_torch(ref, q, c, *inbatch_rowwise.FORMS[form], n_rows_total=n_rows_total)


def score_delta(q, c, form):
    """Per row, the bound of oracle.inbatch_bounds on one score's error:
    eps max_j |q_i| . |c_j| (fp64 [R])."""
    eps = inbatch_rowwise.FORMS[form][0]
    return eps * (q.double().abs() @ c.double().abs().T).max(dim=1).values


def rank_window(Sref, thr, delta, pos_offset=0, row_ids=None, col_ids=None):
    """(lo [R], hi [R]): #(ref S' >= thr + delta) and #(ref S' >= thr - delta)
    over each row's negatives.  A valid thr for rank k has lo <= k <= hi."""
    R, C = Sref.shape
    dev = Sref.device
    rr = torch.arange(R, device=dev)
    V = Sref.masked_fill(hit_matrix(row_ids, col_ids, R, C, dev), NINF).clone()
    V[rr, rr + pos_offset] = NINF
    fin = torch.isfinite(V)
    t = thr.double()[:, None]
    lo = ((V >= t + delta[:, None]) & fin).sum(dim=1)
    hi = ((V >= t - delta[:, None]) & fin).sum(dim=1)
    return lo, hi


# --------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def exact_case(R, C, E, pos_offset=0, hits=False, seed=0):
    """q [R, E], c [C, E] with entries in {-4..4}/8 and logq [C] in multiples
    of 1/64 (numpy float32; ids int32 or None).  Every product is a multiple
    of 1/64 below 1/4 in size and every partial sum a multiple of 1/64 below
    2^11: exact in fp32 in any order, the bf16 residual planes are 0, so the
    kernels' S' equals the fp64 scores bit for bit in both arithmetics.
    Scores take few distinct values: most rows tie at the k-th rank.
    hits: candidate ids with duplicates (row i's id is its positive's)."""
    rng = np.random.default_rng(1000 * R + 10 * C + E + seed)
    q = (rng.integers(-4, 5, (R, E)) / 8.0).astype(np.float32)
    c = (rng.integers(-4, 5, (C, E)) / 8.0).astype(np.float32)
    logq = (rng.integers(-256, 1, C) / 64.0).astype(np.float32)
    row_ids = col_ids = None
    if hits:
        col_ids = rng.integers(0, max(C // 3, 2), C).astype(np.int32)
        row_ids = col_ids[pos_offset:pos_offset + R].copy()
    return {"q": q, "c": c, "logq": logq, "row_ids": row_ids, "col_ids": col_ids, "pos_offset": pos_offset}


GAP_N, GAP_E, GAP_K = 128, 32, 8


@functools.lru_cache(maxsize=None)
def gap_case(seed=7):
    """The end-to-end case (n = 128, E = 32, K = 8): random N(0, 0.05^2)
    operands plus 16 orthonormal directions u_g — candidate j carries
    1.5 u_{j // 8} and query i carries 1.5 u_{(i // 8 + 1) % 16}, so row i
    has exactly 8 negatives near 2.25 (the next group's candidates; its own
    positive sits in group i // 8) over 119 near 0, and the gap a - b clears
    64 delta in the bf16 arithmetic too.  logq in [-0.1, 0]."""
    rng = np.random.default_rng(seed)
    n, E = GAP_N, GAP_E
    u = np.linalg.qr(rng.standard_normal((E, E)))[0][:16]
    g = np.arange(n) // 8
    q = 0.05 * rng.standard_normal((n, E)) + 1.5 * u[(g + 1) % 16]
    c = 0.05 * rng.standard_normal((n, E)) + 1.5 * u[g]
    logq = rng.uniform(-0.1, 0.0, n)
    return {"q": q.astype(np.float32), "c": c.astype(np.float32), "logq": logq.astype(np.float32)}


def to_torch(x, dev):
    return {k: (torch.as_tensor(v, device=dev) if isinstance(v, np.ndarray) else v) for k, v in x.items()}
