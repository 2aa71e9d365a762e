"""Restatements for mixed negative sampling (include/tt.h, "mixed negatives"
and tt_mixed_candidates), shared by tests/test_mixed_neg_host.py and
tests/test_mixed_neg_gpu.py.

  philox4x32_10()  the generator, vectorised numpy (uint32 words)
  sample()         the M catalogue rows of one step: s_m = (u_m * N) >> 32,
                   u_m word m & 3 at counter (m >> 2, step lo, step hi, 0),
                   key (seed lo, seed hi)
  assemble()       tt_mixed_candidates' dst from batch columns and a catalogue
  mixture_logq()   log((B p + M / N) / (B + M)) in fp64
  cols_no_pos_bf16()  the bf16 contract's column pass (oracle.inbatch_cols_bf16)
                   for columns WITHOUT a positive row, with its per-element bound
  case()           loss inputs q [n, E], c [n + m, E], logq, ids
"""
import functools

import numpy as np

from oracle import oracle

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (anything convertible to uint32) ->
    uint32 [..., 4]: ten rounds, the key bumped by the Weyl constants between
    rounds."""
    c = [np.asarray(counter, np.uint64)[..., i] & MASK for i in range(4)]
    k = [np.asarray(key, np.uint64)[..., i] & MASK for i in range(2)]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # < 2^64: exact in uint64
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return np.stack(c, -1).astype(np.uint32)


def words(m, seed, step):
    """u_0 .. u_{m-1} of one step (uint64 holding 32-bit words)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    blocks = (m + 3) // 4
    ctr = np.zeros((blocks, 4), np.uint64)
    ctr[:, 0] = np.arange(blocks)
    ctr[:, 1], ctr[:, 2] = step & MASK, step >> 32
    key = np.array([seed & MASK, seed >> 32], np.uint64)
    return philox4x32_10(ctr, np.broadcast_to(key, (blocks, 2))).reshape(-1)[:m].astype(np.uint64)


def sample(m, n_cat, seed, step):
    """The catalogue rows s_0 .. s_{m-1} (int64) of one step."""
    return ((words(m, seed, step) * np.uint64(n_cat)) >> np.uint64(32)).astype(np.int64)


def assemble(batch_cols, cat, m, seed, step):
    """dst [F, B + m] (the columns' own dtypes kept per row as 32-bit words,
    returned as int32): batch_cols F arrays [B], cat [F, N] int32 words."""
    s = sample(m, cat.shape[1], seed, step)
    rows = [np.concatenate([np.ascontiguousarray(b).view(np.int32), cat[f, s]]) for f, b in enumerate(batch_cols)]
    return np.stack(rows).astype(np.int32)


def mixture_logq(p, B, M, N):
    """fp64 log((B p + M / N) / (B + M))."""
    return np.log((B * np.asarray(p, np.float64) + M / N) / (B + M))


def cols_no_pos_bf16(q_all, lse, c, logq=None, row_ids=None, col_ids=None):
    """oracle.inbatch_cols_bf16's arithmetic for columns that have NO positive
    row (bf16 p and q, fp32 exp2 of the fp32 argument, the exp(-logq) scale),
    and the same per-element bound without the positive's term:
    (dc fp32 [C, E], bound fp64 [C, E])."""
    q32, c32 = np.asarray(q_all, np.float32), np.asarray(c, np.float32)
    R = q32.shape[0]
    qb = oracle.bf16_round(q32).astype(np.float64)
    cb = oracle.bf16_round(c32).astype(np.float64)
    lse64 = np.asarray(lse, np.float32).astype(np.float64)
    sigma = oracle.SOFTMAX_SLACK * (1.0 + np.abs(lse64))
    s = ((qb @ cb.T) - lse64[:, None]).astype(np.float32).astype(np.float64)
    if row_ids is not None:
        s[np.asarray(row_ids)[:, None] == np.asarray(col_ids)[None, :]] = -np.inf
    p = np.exp2((s * oracle.LOG2E_F32).astype(np.float32).astype(np.float64)).astype(np.float32)
    O = oracle.bf16_round(p).astype(np.float64).T @ qb
    w = 2.0 ** -7 + 2.0 * sigma + R * 2.0 ** -24
    Ob = p.astype(np.float64).T @ (w[:, None] * np.abs(qb))
    scale = np.ones(c32.shape[0]) if logq is None else np.exp(-np.asarray(logq, np.float32).astype(np.float64))
    dc = O * scale[:, None]
    bound = Ob * scale[:, None] + 2.0 ** -21 * np.abs(dc) \
        + oracle.FP32_TINY * (1.0 + np.abs(q32.astype(np.float64)).sum(axis=0))[None, :]
    return dc.astype(np.float32), bound


# (n, m) of the kernel tests: (100, 37) the extra columns' would-be positives
# land in the streamed padding; (64, 200) m > n, would-be positives beyond the
# padded streamed extent, several stationary blocks
SHAPES = [(100, 37), (128, 64), (130, 1), (64, 200), (300, 300)]
DIMS = (32, 48, 128)


@functools.lru_cache(maxsize=None)
def case(n, m, E, hits=False, scale=0.15):
    """q [n, E], c [n + m, E] ~ N(0, scale^2) (max |S| far below 16: every row
    certified for the bf16 bounds too), logq ~ log U(1e-6, 1e-2) [n + m], ids
    [n + m] int32 (hits) or None.  hits: ids distinct but for — sampled
    column n duplicates row 3's positive (id, embedding, logq) when m >= 1,
    sampled column n + 1 carries an id of nobody when m >= 2, and batch column
    9 duplicates row 5's positive."""
    rng = np.random.default_rng(977 * n + 31 * m + E)
    q = (rng.standard_normal((n, E)) * scale).astype(np.float32)
    c = (rng.standard_normal((n + m, E)) * scale).astype(np.float32)
    logq = np.log(rng.uniform(1e-6, 1e-2, n + m)).astype(np.float32)
    ids = None
    if hits:
        ids = np.arange(1, n + m + 1, dtype=np.int32)
        c[9], logq[9], ids[9] = c[5], logq[5], ids[5]
        if m >= 1:
            c[n], logq[n], ids[n] = c[3], logq[3], ids[3]
        if m >= 2:
            ids[n + 1] = 1 << 20
    return {"q": q, "c": c, "logq": logq, "ids": ids}
