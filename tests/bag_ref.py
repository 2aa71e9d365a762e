"""numpy restatement of the pooled embedding bags (tt_gather_bag,
tt_bag_grad_expand; contract in include/tt.h) and of the flat sparse problem
they hand to the optimizer.  fp32 throughout, one IEEE operation per step, in
the kernel's order: the sum runs over the valid slots in slot order and the
first valid row starts it."""
import numpy as np

from oracle import oracle

POOLINGS = ("sum", "mean", "sqrtn")


def valid_slots(ids: np.ndarray, num_rows: int) -> np.ndarray:
    ids = np.asarray(ids)
    return (ids >= 0) & (ids < num_rows)


def bag_scale(cnt: np.ndarray, pooling: str) -> np.ndarray:
    """1 (sum), 1 / cnt (mean), 1 / sqrt(cnt) (sqrtn) in fp32; 0 where cnt == 0."""
    n = np.maximum(cnt, 1).astype(np.float32)
    one = np.float32(1.0)
    if pooling == "sum":
        s = np.ones_like(n)
    elif pooling == "mean":
        s = one / n
    elif pooling == "sqrtn":
        s = one / np.sqrt(n)
    else:
        raise ValueError(pooling)
    return np.where(cnt > 0, s, np.float32(0.0)).astype(np.float32)


def gather_bag(table: np.ndarray, ids: np.ndarray, pooling: str):
    """table [V, D] fp32, ids [B, L] -> (out [B, D] fp32, scale [B] fp32)."""
    table = np.ascontiguousarray(table, np.float32)
    ids = np.asarray(ids)
    B, L = ids.shape
    ok = valid_slots(ids, table.shape[0])
    s = np.zeros((B, table.shape[1]), np.float32)
    started = np.zeros(B, bool)
    for l in range(L):
        rows = table[np.where(ok[:, l], ids[:, l], 0)]
        nxt = np.where(started[:, None], s + rows, rows)
        s = np.where(ok[:, l][:, None], nxt, s)
        started |= ok[:, l]
    cnt = ok.sum(1)
    scale = bag_scale(cnt, pooling)
    out = s if pooling == "sum" else s * scale[:, None]
    out = np.where((cnt > 0)[:, None], out, np.float32(0.0)).astype(np.float32)
    return out, scale


def expand(ids: np.ndarray, num_rows: int, dout: np.ndarray, scale: np.ndarray, pooling: str):
    """(ids_flat [B * L] int32, G [B * L, D] fp32, valid [B * L] bool); rows of
    G at invalid lookups are zero here and unspecified in the kernel's output."""
    ids = np.asarray(ids)
    B, L = ids.shape
    ok = valid_slots(ids, num_rows)
    ids_flat = np.where(ok, ids, -1).astype(np.int32).reshape(-1)
    dout = np.asarray(dout, np.float32)
    g = dout if pooling == "sum" else dout * np.asarray(scale, np.float32)[:, None]
    G = np.repeat(g.astype(np.float32), L, axis=0)
    valid = ok.reshape(-1)
    G[~valid] = 0.0
    return ids_flat, G, valid


def flat_adagrad(table, accum, ids_flat, G, lr, eps):
    """The table update: the existing sparse Adagrad on the flat problem (in place)."""
    oracle.sparse_adagrad(table, accum, ids_flat, G, lr, eps)


def flat_adam(table, m, v, ids_flat, G, lr, beta1, beta2, eps, step):
    oracle.sparse_adam(table, m, v, ids_flat, G, lr, beta1, beta2, eps, step)


def random_bags(rng: np.random.Generator, B: int, L: int, num_rows: int) -> np.ndarray:
    """[B, L] int32 bags exercising every kind of slot: left-aligned histories
    of every length 0..L padded with -1, ids >= num_rows, negative ids other
    than -1, padding in the middle, duplicates inside a bag and row 0."""
    ids = rng.integers(0, num_rows, (B, L)).astype(np.int32)
    length = rng.integers(0, L + 1, B)
    length[0] = 0                      # empty bag
    length[-1] = L                     # full bag
    ids[np.arange(L)[None, :] >= length[:, None]] = -1
    r = rng.random((B, L))
    ids[r < 0.06] = num_rows + rng.integers(0, 5)   # out of range above
    ids[(r >= 0.06) & (r < 0.10)] = -7              # negative, not the padding id
    ids[(r >= 0.10) & (r < 0.16)] = 0               # the OOV row
    if L > 1:
        dup = rng.random(B) < 0.4
        ids[dup, 1] = ids[dup, 0]                   # duplicates inside a bag
    ids[0] = -1                        # the empty bag stays all padding
    if B > 2:
        ids[1] =np.where(np.arange(L) % 2 == 0, -1, num_rows)  # nothing valid, not all padding
    return ids
