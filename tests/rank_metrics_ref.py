"""The contract of tt_rank_metrics (include/tt.h) restated in numpy, and a
deliberately naive Python double loop to check the restatement against.

rank_metrics: per-query recall / ap / ndcg / rr at every k in fp32 with the
stated operation order, hits@k and m.
reduce_acc:   the accumulators' 256-lane fp64 reduction.
naive:        one query, nothing but loops and comparisons.
"""
import numpy as np

PAD = 0x7FFFFFFF


def tables(k_list):
    """disc[i] = float32(1 / log2(i + 2)) from float64; idcg[n] = sequential fp32 sum of disc[:n]."""
    disc = np.empty(k_list, np.float32)
    idcg = np.zeros(k_list + 1, np.float32)
    for i in range(k_list):
        disc[i] = np.float32(1.0 / np.log2(np.float64(i + 2)))
        idcg[i + 1] = np.float32(idcg[i] + disc[i])  # one fp32 add
    assert np.array_equal(idcg[1:], np.cumsum(disc, dtype=np.float32))
    return disc, idcg


def _valid(a):
    return (a >= 0) & (a != PAD)


def rank_metrics(cand, truth, ks):
    """cand [Q, k_list] int32, truth [Q, T] int32 -> (vals [Q, nk, 4] fp32 =
    recall, ap, ndcg, rr; hits [Q, nk] int32; m [Q] int32)."""
    cand, truth = np.asarray(cand, np.int32), np.asarray(truth, np.int32)
    Q, k_list = cand.shape
    disc, idcg = tables(k_list)
    nk = len(ks)
    vals = np.zeros((Q, nk, 4), np.float32)
    hits = np.zeros((Q, nk), np.int32)
    m_out = np.zeros(Q, np.int32)
    for q in range(Q):
        want = np.unique(truth[q][_valid(truth[q])])
        m = int(want.size)
        m_out[q] = m
        if m == 0:
            continue
        row = cand[q]
        first = np.zeros(k_list, bool)
        first[np.unique(row, return_index=True)[1]] = True  # the first position of every value
        h = first & _valid(row) & np.isin(row, want)
        pos = np.flatnonzero(h)  # 0-based hit positions, ascending
        c_at = np.arange(1, pos.size + 1)
        ap_run = np.cumsum(c_at.astype(np.float32) / (pos + 1).astype(np.float32), dtype=np.float32)
        dcg_run = np.cumsum(disc[pos], dtype=np.float32)
        for j, k in enumerate(ks):
            c = int(np.searchsorted(pos, k))  # hits at positions < k
            mk = min(m, k)
            ap = ap_run[c - 1] if c else np.float32(0)
            dcg = dcg_run[c - 1] if c else np.float32(0)
            rr = np.float32(1) / np.float32(pos[0] + 1) if c else np.float32(0)
            vals[q, j] = (np.float32(c) / np.float32(m), ap / np.float32(mk), dcg / idcg[mk], rr)
            hits[q, j] = c
    return vals, hits, m_out


def naive(cand_row, truth_row, ks):
    """One query by loops alone -> ([(recall, ap, ndcg, rr)] per k, [hits] per k, m)."""
    cand_row, truth_row = [int(v) for v in cand_row], [int(v) for v in truth_row]
    want = []
    for v in truth_row:
        if v < 0 or v == PAD:
            continue
        dup = False
        for w in want:
            if w == v:
                dup = True
        if not dup:
            want.append(v)
    m = len(want)
    out_v, out_h = [], []
    for k in ks:
        if m == 0:
            out_v.append((np.float32(0),) * 4)
            out_h.append(0)
            continue
        c, first = 0, 0
        ap, dcg = np.float32(0), np.float32(0)
        for i in range(1, k + 1):
            v = cand_row[i - 1]
            if v < 0 or v == PAD:
                continue
            member = False
            for w in want:
                if w == v:
                    member = True
            earlier = False
            for i2 in range(1, i):
                if cand_row[i2 - 1] == v:
                    earlier = True
            if member and not earlier:
                c += 1
                ap = np.float32(ap + np.float32(np.float32(c) / np.float32(i)))
                dcg = np.float32(dcg + np.float32(1.0 / np.log2(np.float64(i + 1))))
                if first == 0:
                    first = i
        ideal = np.float32(0)
        for n in range(1, min(m, k) + 1):
            ideal = np.float32(ideal + np.float32(1.0 / np.log2(np.float64(n + 1))))
        out_v.append((np.float32(c) / np.float32(m), np.float32(ap / np.float32(min(m, k))),
                      np.float32(dcg / ideal), np.float32(1) / np.float32(first) if first else np.float32(0)))
        out_h.append(c)
    return out_v, out_h, m


def reduce_acc(vals, hits, m, acc=None):
    """The second launch: per (j, metric), lane t of 256 adds the fp32 values
    of queries t, t + 256, ... in ascending order as doubles, skipping m = 0;
    x[t] += x[t + s] for s = 128 .. 1; acc += x[0].  acc = (acc_f64 [nk, 4],
    acc_i64 [nk, 2], n_valid [1]) or None for zeros; returns new arrays."""
    Q, nk, _ = vals.shape
    if acc is None:
        acc = (np.zeros((nk, 4), np.float64), np.zeros((nk, 2), np.int64), np.zeros(1, np.int64))
    f64, i64, n_valid = (a.copy() for a in acc)
    scored = m > 0
    rows = -(-Q // 256)
    for j in range(nk):
        for metric in range(4):
            col = np.zeros(rows * 256, np.float64)
            col[:Q] = np.where(scored, vals[:, j, metric].astype(np.float64), 0.0)
            skip = np.ones(rows * 256, bool)
            skip[:Q] = ~scored
            x = np.zeros(256, np.float64)
            for r in range(rows):  # lane t's r-th query is r * 256 + t
                sl = slice(r * 256, (r + 1) * 256)
                x = np.where(skip[sl], x, x + col[sl])
            s = 128
            while s >= 1:
                x[:s] = x[:s] + x[s:2 * s]
                s //= 2
            f64[j, metric] = f64[j, metric] + x[0]
        i64[j, 0] += int(hits[scored, j].astype(np.int64).sum())
        i64[j, 1] += int((hits[scored, j] > 0).sum())
    n_valid[0] += int(scored.sum())
    return f64, i64, n_valid
