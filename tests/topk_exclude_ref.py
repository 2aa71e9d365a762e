"""numpy restatement of the exact top-k with per-query exclusions, written
independently of the kernel's hash scheme (Python sets and a full sort).

exclude_lists: tt_topk_exclude's contract on sorted lists.
filtered_topk: the exact filtered top-k of a whole problem from the fp32
fmaf-chain scores (oracle.fmaf_scores), ordered (score desc, index asc).
"""
import numpy as np

PAD_INDEX = 0x7FFFFFFF


def exclude_lists(scores, idx, excl_off, excl_idx, k_out):
    """Per query: drop the list entries whose index is in set(E_q), keep the
    order, write the first k_out, pad the tail with (-inf, PAD_INDEX).
    Negative exclusions and PAD_INDEX match nothing.  Returns (scores
    [Q, k_out] float32, idx [Q, k_out] int32, n_kept [Q] int32, survivors [Q]:
    the kept entries before the cut at k_out)."""
    scores = np.asarray(scores, np.float32)
    idx = np.asarray(idx, np.int32)
    excl_off = np.asarray(excl_off, np.int64)
    excl_idx = np.asarray(excl_idx, np.int64)
    Q, _ = scores.shape
    out_s = np.full((Q, k_out), -np.inf, np.float32)
    out_i = np.full((Q, k_out), PAD_INDEX, np.int32)
    kept = np.zeros(Q, np.int32)
    survivors = np.zeros(Q, np.int64)
    for q in range(Q):
        gone = {int(v) for v in excl_idx[excl_off[q]:excl_off[q + 1]] if 0 <= v != PAD_INDEX}
        stay = [j for j in range(idx.shape[1]) if int(idx[q, j]) not in gone]
        survivors[q] = len(stay)
        stay = stay[:k_out]
        kept[q] = len(stay)
        out_s[q, :len(stay)] = scores[q, stay]
        out_i[q, :len(stay)] = idx[q, stay]
    return out_s, out_i, kept, survivors


def csr_of(rows):
    """(off int64 [Q + 1], idx int32 [total]) of a list of per-query lists."""
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    flat = np.concatenate([np.asarray(r, np.int64).reshape(-1) for r in rows]) if rows else np.zeros(0, np.int64)
    return off, flat.astype(np.int32)


def filtered_topk(all_scores, rows, k):
    """all_scores [Q, N] (oracle.fmaf_scores); rows: per-query excluded
    columns.  (scores [Q, k], idx [Q, k]) of the remaining columns ordered
    (score desc, index asc), padded with (-inf, PAD_INDEX) when fewer than k
    remain."""
    all_scores = np.asarray(all_scores, np.float32)
    Q, N = all_scores.shape
    out_s = np.full((Q, k), -np.inf, np.float32)
    out_i = np.full((Q, k), PAD_INDEX, np.int32)
    for q in range(Q):
        gone = {int(v) for v in rows[q] if 0 <= int(v) < N}
        cols = np.array([j for j in range(N) if j not in gone], np.int64)
        s = all_scores[q, cols]
        order = np.lexsort((cols, -s.astype(np.float64)))[:k]
        out_s[q, :order.size] = s[order]
        out_i[q, :order.size] = cols[order]
    return out_s, out_i
