"""IndexRankingMetrics: MAP@K, NDCG@K, MRR, recall@K, hit rate and precision@K
of an index against SET-valued ground truth (the H&M task scores MAP@12 over
the set of articles a customer buys in the following week).

Per query, with m = the number of distinct valid true ids, position i
(1-based) a hit when the list's entry is a true id and i is the first position
holding it, and c_i the hits up to i:

    recall@k = c_k / m
    ap@k     = (sum over hits i <= k of c_i / i) / min(m, k)
    ndcg@k   = (sum over hits i <= k of 1 / log2(i + 1)) / (sum over i <= min(m, k) of 1 / log2(i + 1))
    rr@k     = 1 / (first hit) when it is <= k, else 0

in fp32, sums sequential in ascending i (include/tt.h, tt_rank_metrics).  A
query without a true id is not scored (the Kaggle convention): it counts in
`.skipped`, never in an average.  With integer identifiers on the GPU a batch
is one libtt call (hip_ops.rank_metrics) that accumulates on the device until
read; string identifiers take the host path below, with the same definitions.
Integer identifiers are compared as int32, like IndexRecall's; negative values
and INT32_MAX are padding.
"""
from __future__ import annotations

import logging
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from pkg.modelling import hip_ops

logger = logging.getLogger(__name__)

__all__ = ["IndexRankingMetrics", "host_rank_metrics"]

PAD_INDEX = 0x7FFFFFFF
METRICS = ("recall", "map", "ndcg", "mrr", "hit_rate", "precision")


def _plain(x):
    if isinstance(x, bytes):
        return x.decode()
    if isinstance(x, (np.generic, torch.Tensor)):
        return x.item()
    return x


def _is_padding(x) -> bool:
    if x is None or x == "":
        return True
    return isinstance(x, (int, np.integer)) and (x < 0 or x == PAD_INDEX)


def host_rank_metrics(cand_rows, truth_rows, ks: Sequence[int]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """tt_rank_metrics on the host, for identifiers of any hashable type:
    (vals [Q, len(ks), 4] fp32 = recall, ap, ndcg, rr; hits [Q, len(ks)]
    int32; m [Q] int32).  None, "" and, for integers, negative values and
    INT32_MAX are padding."""
    if isinstance(cand_rows, np.ndarray) and cand_rows.dtype.kind in "iu":
        cand_rows = cand_rows.tolist()  # Python ints already
    else:
        cand_rows = [[_plain(x) for x in row] for row in cand_rows]
    if isinstance(truth_rows, np.ndarray) and truth_rows.dtype.kind in "iu":
        truth_rows = truth_rows.tolist()
    k_list = max((len(r) for r in cand_rows), default=0)
    disc, idcg = hip_ops.rank_discount_tables(max(k_list, 1))
    Q, nk = len(cand_rows), len(ks)
    vals = np.zeros((Q, nk, 4), np.float32)
    hits = np.zeros((Q, nk), np.int32)
    m_out = np.zeros(Q, np.int32)
    for q, (row, truth) in enumerate(zip(cand_rows, truth_rows)):
        want = {x for x in (_plain(t) for t in truth) if not _is_padding(x)}
        m = len(want)
        m_out[q] = m
        if m == 0:
            continue
        found, hitpos = set(), []
        for i, x in enumerate(row):
            if x in want and x not in found:  # `want` holds no padding value
                found.add(x)
                hitpos.append(i)
        for j, k in enumerate(ks):
            c, ap, dcg = 0, np.float32(0), np.float32(0)
            for p in hitpos:
                if p >= k:
                    break
                c += 1
                ap = ap + np.float32(c) / np.float32(p + 1)
                dcg = dcg + disc[p]
            mk = min(m, k)
            first = hitpos[0] + 1 if c else 0
            vals[q, j] = (np.float32(c) / np.float32(m), ap / np.float32(mk), dcg / idcg[mk],
                          np.float32(1) / np.float32(first) if first else np.float32(0))
            hits[q, j] = c
    return vals, hits, m_out


def _is_row(x) -> bool:
    return isinstance(x, (list, tuple, np.ndarray)) or (isinstance(x, torch.Tensor) and x.dim() > 0)


class IndexRankingMetrics:
    """
    Given an index, calculate ranking metrics at several K against a SET of
    true candidates per query.

    Parameters
    ----------
    index: BruteForceIndex | StaticIndex | sharded index | callable
        Maps a query feature dict to [B, K] candidate identifiers.
    ks: List[int]
        The top Ks to calculate the metrics at (each <= the index's K).
    """

    def __init__(self, index, ks: List[int]):
        self.index = index
        self.ks = [int(k) for k in ks]
        if not 1 <= len(self.ks) <= 16 or min(self.ks) < 1:
            raise ValueError(f"need 1 to 16 values of k, each >= 1, got {ks}")
        nk = len(self.ks)
        self._host_f64 = np.zeros((nk, 4), np.float64)
        self._host_i64 = np.zeros((nk, 2), np.int64)
        self._host_valid = 0
        self._dev_acc: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None
        self.total = 0  # queries passed in, scored or not

    # ------------------------------------------------------------------ truth forms
    @staticmethod
    def _device_truth(true_ids, n: int, device: torch.device) -> torch.Tensor:
        """[n, T] int32 on `device`, padded with -1."""
        if isinstance(true_ids, (list, tuple)) and any(_is_row(r) for r in true_ids):
            rows = [np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r, dtype=np.int64).reshape(-1)
                    for r in true_ids]
            t = np.full((len(rows), max(1, max((r.size for r in rows), default=1))), -1, np.int64)
            for q, r in enumerate(rows):
                t[q, :r.size] = r
            true_ids = t
        t = torch.as_tensor(true_ids)
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise TypeError(f"true ids must be integers, got {t.dtype}")
        t = t.reshape(n, -1) if t.dim() != 2 else t
        if t.shape[0] != n:
            raise ValueError(f"true ids have {t.shape[0]} rows, the index returned {n}")
        if t.dtype != torch.int32:  # identifiers past int32 must not wrap into padding or another id
            t = t.to(device)
            t = torch.where((t < 0) | (t >= PAD_INDEX), torch.full_like(t, -1), t)
        return t.to(device, torch.int32).contiguous()

    @staticmethod
    def _host_truth(true_ids, n: int) -> List[Sequence[Any]]:
        if isinstance(true_ids, torch.Tensor):
            true_ids = true_ids.cpu().numpy()
        if isinstance(true_ids, np.ndarray) and not (true_ids.dtype == object and true_ids.ndim == 1
                                                     and any(_is_row(r) for r in true_ids)):
            rows = [r.reshape(-1).tolist() for r in true_ids.reshape(n, -1)]
        else:
            rows = [list(r) if _is_row(r) else [r] for r in true_ids]
        if len(rows) != n:
            raise ValueError(f"true ids have {len(rows)} rows, the index returned {n}")
        return rows

    # ------------------------------------------------------------------ accumulation
    def _update(self, true_ids, candidates) -> None:
        if not isinstance(candidates, torch.Tensor):
            candidates = np.asarray(candidates)
        n, width = int(candidates.shape[0]), int(candidates.shape[1])
        if max(self.ks) > width:
            raise ValueError(f"k={max(self.ks)} exceeds the {width} candidates the index returns")
        self.total += n
        if n == 0:
            return
        if (isinstance(candidates, torch.Tensor) and candidates.device.type == "cuda"
                and candidates.dtype in (torch.int32, torch.int64)):
            c = candidates
            if c.dtype != torch.int32:  # as for the true ids: nothing wraps into another id
                c = torch.where((c < 0) | (c >= PAD_INDEX), torch.full_like(c, -1), c).to(torch.int32)
            c = c.contiguous()
            t = self._device_truth(true_ids, n, c.device)
            if self._dev_acc is None:
                nk = len(self.ks)
                self._dev_acc = (torch.zeros(nk, 4, dtype=torch.float64, device=c.device),
                                 torch.zeros(nk, 2, dtype=torch.int64, device=c.device),
                                 torch.zeros(1, dtype=torch.int64, device=c.device))
            hip_ops.rank_metrics(c, t, self.ks, self._dev_acc)
        else:
            c = candidates.cpu().numpy() if isinstance(candidates, torch.Tensor) else np.asarray(candidates)
            vals, hits, m = host_rank_metrics(c, self._host_truth(true_ids, n), self.ks)
            scored = m > 0
            self._host_f64 += vals[scored].astype(np.float64).sum(0)
            self._host_i64[:, 0] += hits[scored].astype(np.int64).sum(0)
            self._host_i64[:, 1] += (hits[scored] > 0).sum(0)
            self._host_valid += int(scored.sum())

    def update(self, queries: Dict[str, Any], true_ids, exclusions=None) -> None:
        """Score one batch without reading the device accumulators back."""
        candidates = self.index(queries) if exclusions is None else self.index(queries, exclusions=exclusions)
        self._update(true_ids, candidates)

    def __call__(self, queries: Dict[str, Any], true_ids, exclusions=None) -> Dict[str, Dict[int, np.float64]]:
        """true_ids: an integer [B, T] tensor / array padded with -1, a [B]
        vector (one true id per query), or a list of per-query lists.
        exclusions: per-query identifiers the index must leave out (metrics on
        unseen items), forwarded as index(queries, exclusions=...)."""
        self.update(queries, true_ids, exclusions)
        return self.metric

    # ------------------------------------------------------------------ reading
    def _totals(self) -> Tuple[np.ndarray, np.ndarray, int]:
        f, i, v = self._host_f64.copy(), self._host_i64.copy(), self._host_valid
        if self._dev_acc is not None:
            f += self._dev_acc[0].cpu().numpy()
            i += self._dev_acc[1].cpu().numpy()
            v += int(self._dev_acc[2].item())
        return f, i, v

    @property
    def seen(self) -> int:
        """Scored queries (those with at least one true id)."""
        return self._totals()[2]

    @property
    def skipped(self) -> int:
        """Queries left out of every average (no true id)."""
        return self.total - self.seen

    @property
    def hits(self) -> Dict[int, int]:
        return {k: int(v) for k, v in zip(self.ks, self._totals()[1][:, 0])}

    @property
    def metric(self) -> Dict[str, Dict[int, np.float64]]:
        f, i, v = self._totals()
        out: Dict[str, Dict[int, np.float64]] = {name: {} for name in METRICS}
        for j, k in enumerate(self.ks):
            n = np.float64(v)
            for col, name in enumerate(("recall", "map", "ndcg", "mrr")):
                out[name][k] = np.float64(f[j, col]) / n if v else np.float64(0.0)
            out["hit_rate"][k] = np.float64(i[j, 1]) / n if v else np.float64(0.0)
            out["precision"][k] = np.float64(i[j, 0]) / (np.float64(k) * n) if v else np.float64(0.0)
        return out

    def log_metric(self, epoch: Optional[int] = None, to_tensorboard: bool = True) -> None:
        m = self.metric
        for name in METRICS:
            for k in self.ks:
                logger.info(f"Start of epoch {epoch} {name}@{k}: {m[name][k]}")
