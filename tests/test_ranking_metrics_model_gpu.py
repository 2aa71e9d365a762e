"""GPU: IndexRankingMetrics over a BruteForceIndex, each value against one that
does not come from the code under test: the numpy restatement
(tests/rank_metrics_ref.py) applied to a numpy top-k of the fp32 fmaf-chain
scores (plain and with exclusions), and IndexRecall for single true ids."""
import functools

import numpy as np
import pytest
import torch

import rank_metrics_ref as ref
import topk_exclude_ref as xref
from oracle import oracle
from pkg.modelling.indices.brute_force import BruteForceIndex
from pkg.modelling.metrics import IndexRankingMetrics
from pkg.modelling.metrics.index_recall import IndexRecall

N, E, Q, K = 300, 16, 64, 100
KS = [1, 12, 100]


def _ident(pos):
    return 3 * np.asarray(pos, np.int64) + 11


@functools.lru_cache(maxsize=None)
def _problem():
    """Candidates, queries, the fp32 score matrix, truth sets of 0-5 ids drawn
    mostly from each query's own top-150, and exclusions that bite."""
    rng = np.random.default_rng(5)
    c = rng.standard_normal((N, E)).astype(np.float32)
    q = rng.standard_normal((Q, E)).astype(np.float32)
    full = oracle.fmaf_scores(q, c)
    _, top = xref.filtered_topk(full, [[]] * Q, 150)
    truth, excl = [], []
    for b in range(Q):
        n = b % 6  # 0 .. 5 true ids
        t = rng.choice(top[b], n, replace=False).tolist()
        if n >= 3:
            t[0] = int(rng.integers(N))  # anywhere in the catalogue
        if n == 5:
            t[4] = t[1]                  # a repeated true id: m = 4
        truth.append([int(v) for v in t])
        # what the customer has already: some of the best candidates, never a true id
        e = [int(v) for v in top[b, :8 + b % 5] if int(v) not in t][:b % 7]
        excl.append(e)
    for a in (c, q, full):
        a.setflags(write=False)
    return c, q, full, truth, excl


def _padded(rows, fill=-1):
    out = np.full((len(rows), max(1, max(len(r) for r in rows))), fill, np.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def _expected(lists, truth_rows):
    """{metric: {k: float64}} from the restatement over position lists and position truth."""
    vals, hits, m = ref.rank_metrics(lists, _padded(truth_rows), KS)
    f64, i64, nv = ref.reduce_acc(vals, hits, m)
    n = np.float64(nv[0])
    out = {name: {k: np.float64(f64[j, c]) / n for j, k in enumerate(KS)}
           for c, name in enumerate(("recall", "map", "ndcg", "mrr"))}
    out["hit_rate"] = {k: np.float64(i64[j, 1]) / n for j, k in enumerate(KS)}
    out["precision"] = {k: np.float64(i64[j, 0]) / (np.float64(k) * n) for j, k in enumerate(KS)}
    return out, int(nv[0])


def _index(cuda, c):
    return BruteForceIndex(K, lambda x: x["emb"], [(torch.as_tensor(_ident(np.arange(N))), torch.tensor(c))],
                           device=cuda)


@pytest.mark.gpu
def test_plain_evaluation_equals_the_restatement_on_a_numpy_topk(cuda):
    c, q, full, truth, _ = _problem()
    _, lists = xref.filtered_topk(full, [[]] * Q, K)
    want, n = _expected(lists, truth)
    assert 0 < n < Q and 0 < want["map"][12] < 1
    index = _index(cuda, c)
    queries = {"emb": torch.tensor(q, device=cuda)}
    by_id = [[int(v) for v in _ident(r)] for r in truth]
    m = IndexRankingMetrics(index, KS)
    assert m(queries, by_id) == want                       # a list of per-query lists
    assert m.seen == n and m.skipped == Q - n and m.total == Q
    for form in (torch.as_tensor(np.where(_padded(truth) < 0, -1, _ident(_padded(truth)))),   # [B, T] int64, CPU
                 torch.as_tensor(np.where(_padded(truth) < 0, -1, _ident(_padded(truth))), device=cuda).int()):
        m2 = IndexRankingMetrics(index, KS)
        assert m2(queries, form) == want
    # two halves accumulate on the device to the restated two-step sums
    m3 = IndexRankingMetrics(index, KS)
    m3.update({"emb": queries["emb"][:40]}, by_id[:40])
    m3.update({"emb": queries["emb"][40:]}, by_id[40:])
    v1 = ref.rank_metrics(lists[:40], _padded(truth[:40]), KS)
    v2 = ref.rank_metrics(lists[40:], _padded(truth[40:]), KS)
    f64, i64, nv = ref.reduce_acc(*v2, ref.reduce_acc(*v1))
    assert m3.seen == nv[0] and m3.metric["ndcg"][12] == np.float64(f64[1, 2]) / np.float64(nv[0])
    assert m3.hits == {k: int(i64[j, 0]) for j, k in enumerate(KS)}


@pytest.mark.gpu
def test_evaluation_with_exclusions_equals_the_filtered_numpy_topk(cuda):
    c, q, full, truth, excl = _problem()
    _, lists = xref.filtered_topk(full, excl, K)
    _, plain = xref.filtered_topk(full, [[]] * Q, K)
    assert not np.array_equal(lists, plain)  # the exclusions bite
    want, n = _expected(lists, truth)
    m = IndexRankingMetrics(_index(cuda, c), KS)
    got = m({"emb": torch.tensor(q, device=cuda)}, [[int(v) for v in _ident(r)] for r in truth],
            exclusions=[[int(v) for v in _ident(r)] for r in excl])
    assert got == want and m.seen == n
    assert got != _expected(plain, truth)[0]


@pytest.mark.gpu
def test_single_true_ids_give_index_recalls_metric(cuda):
    c, q, full, _, _ = _problem()
    rng = np.random.default_rng(6)
    _, top = xref.filtered_topk(full, [[]] * Q, 200)
    true = _ident(top[np.arange(Q), rng.integers(0, 200, Q)])  # half of them outside the top-100
    index = _index(cuda, c)
    queries = {"emb": torch.tensor(q, device=cuda)}
    a, b = IndexRankingMetrics(index, KS), IndexRecall(index, KS)
    ra, rb = a(queries, torch.as_tensor(true)), b(queries, torch.as_tensor(true))
    assert ra["recall"] == rb and ra["hit_rate"] == rb and a.hits == b.hits and a.seen == b.seen == Q
    assert 0 < rb[100] < 1
