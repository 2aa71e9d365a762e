"""Host planning of the exact top-k with per-query exclusions (TensorFlow
Recommenders' `query_with_exclusions`).

The exact search is run at k' = k + (the query's exclusion count) and
tt_topk_exclude removes the excluded candidates from each sorted list and
compacts it to k.  This is exact by construction: the top-k' minus at most
k' - k removed entries leaves the true top-k of the remaining candidates, in
the same order (score descending, ties to the lower index).

To keep k' close to each query's own count, the queries of a batch are
grouped into at most six classes by exclusion count (0, <= 16, <= 64, <= 256,
<= 1024, more) and each class is searched at k' = min(k + the class's largest
count, n_candidates).  The class of count 0 is answered by the plain search
and returns its bits.  k + count <= 4000, the bound of tt_bruteforce_search.

Everything here is torch / numpy on whatever device the inputs live on: no
libtt call, importable and testable without a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

__all__ = ["K_LIMIT", "CLASS_BOUNDS", "ExclusionClass", "as_csr", "plan_classes", "take_rows", "drop_negative",
           "IdentifierMap", "positions_of", "identifier_csr", "run_classes"]

K_LIMIT = 4000                      # tt_bruteforce_search: k <= 4000
CLASS_BOUNDS = (0, 16, 64, 256, 1024)  # largest count of each class but the last ("more")


def _is_array(x) -> bool:
    return isinstance(x, (torch.Tensor, np.ndarray))


def _as_tensor(x, dtype: torch.dtype) -> torch.Tensor:
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.is_floating_point() or t.dtype == torch.bool:
        raise TypeError(f"exclusions must be integers, got {t.dtype}")
    return t.to(dtype)


def _offsets(counts: torch.Tensor) -> torch.Tensor:
    off = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    torch.cumsum(counts, 0, out=off[1:])
    return off


def as_csr(exclusions, n_queries: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(off int64 [n_queries + 1], idx int32 [total], counts int64 [n_queries])
    of per-query exclusions given as candidate positions in one of three forms:

    * a [n_queries, E] integer tensor / array padded with negative values
      (the padding is dropped);
    * a sequence (list) of n_queries per-query sequences;
    * an (off, idx) pair: a *tuple* of two tensors / arrays, off [n_queries +
      1] starting at 0, non-decreasing and ending at len(idx).

    Tensors stay on their device; the other forms come back on the CPU.
    counts[q] = off[q + 1] - off[q] may include duplicates and positions that
    match nothing: the counts only need to be upper bounds on what a query
    removes."""
    n = int(n_queries)
    if isinstance(exclusions, tuple) and len(exclusions) == 2 and all(_is_array(x) for x in exclusions):
        off, idx = _as_tensor(exclusions[0], torch.int64).reshape(-1), _as_tensor(exclusions[1], torch.int32)
        idx = idx.reshape(-1).to(off.device)
        if off.numel() != n + 1:
            raise ValueError(f"exclusion offsets must have {n + 1} entries, got {off.numel()}")
        counts = off[1:] - off[:-1]
        ok = (off[0] == 0) & (off[-1] == idx.numel()) & (counts >= 0).all()
        if not bool(ok):  # checked on the host: the kernel trusts the offsets
            raise ValueError("exclusion offsets must start at 0, be non-decreasing and end at len(idx)")
        return off.contiguous(), idx.contiguous(), counts
    if _is_array(exclusions):
        x = _as_tensor(exclusions, torch.int32)
        if x.dim() != 2 or x.shape[0] != n:
            raise ValueError(f"padded exclusions must be [{n}, E], got shape {tuple(x.shape)}")
        keep = x >= 0
        counts = keep.sum(1, dtype=torch.int64)
        return _offsets(counts), x[keep].contiguous(), counts
    rows = list(exclusions)
    if len(rows) != n:
        raise ValueError(f"need one exclusion list per query ({n}), got {len(rows)}")
    rows = [np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r).reshape(-1) for r in rows]
    for r in rows:
        if r.size and r.dtype.kind not in "iu":
            raise TypeError(f"exclusions must be integers, got {r.dtype}")
    counts = torch.as_tensor([r.size for r in rows], dtype=torch.int64).reshape(-1)
    flat = np.concatenate([r.astype(np.int64) for r in rows]) if rows else np.zeros(0, np.int64)
    return _offsets(counts), torch.as_tensor(flat.astype(np.int32)), counts


@dataclass
class ExclusionClass:
    """Queries `rows` (ascending int64 positions in the batch) are searched at
    k_search; `count` is the largest exclusion count among them (0: the plain
    search answers them) and `total` the sum of their counts."""
    rows: torch.Tensor
    k_search: int
    count: int
    total: int


def plan_classes(counts, k: int, n_candidates: int, k_max: int = K_LIMIT) -> List[ExclusionClass]:
    """Group the queries by exclusion count into at most six classes (0,
    <= 16, <= 64, <= 256, <= 1024, more), each searched at k' = min(k + its
    largest count, n_candidates); empty classes are left out, and a batch
    without any exclusion (or without any query) is one class with k' = k.
    Raises ValueError when k + a count exceeds k_max (4000, the bound of
    tt_bruteforce_search).

    The split reads the counts on the host: one synchronisation per call when
    they live on the device.  That is acceptable because the search is not
    graph-captured."""
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    c = c.reshape(-1).astype(np.int64)  # numpy: a few small arrays, far lighter than torch ops
    k, n_candidates = int(k), int(n_candidates)
    if not 1 <= k <= n_candidates:
        raise ValueError(f"need 1 <= k <= n_candidates = {n_candidates}, got k={k}")
    top = int(c.max()) if c.size else 0
    if k + top > k_max:
        raise ValueError(f"k + exclusions = {k} + {top} exceeds the search limit of {k_max} results per query")
    if top == 0:
        return [ExclusionClass(torch.arange(c.size, dtype=torch.int64), k, 0, 0)]
    cls = np.searchsorted(np.asarray(CLASS_BOUNDS), c)  # count <= bound[cls]; 5: more
    out = []
    for j in np.unique(cls):
        rows = np.flatnonzero(cls == j)
        cj = c[rows]
        out.append(ExclusionClass(torch.from_numpy(rows), min(k + int(cj.max()), n_candidates), int(cj.max()),
                                  int(cj.sum())))
    return out


def take_rows(off: torch.Tensor, idx: torch.Tensor, rows: torch.Tensor,
              total: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The CSR (off, idx) of the queries `rows`, in that order.  total: the
    sum of their counts when the host already knows it (no synchronisation)."""
    rows = rows.to(off.device)
    begin = off[rows]
    lens = off[rows + 1] - begin
    new_off = _offsets(lens)
    if total is None:
        total = int(new_off[-1])
    src = torch.repeat_interleave(begin - new_off[:-1], lens, output_size=total) + torch.arange(
        total, dtype=torch.int64, device=off.device)
    return new_off, idx[src].contiguous()


def drop_negative(off: torch.Tensor, idx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The CSR without its negative entries (identifiers the index does not hold)."""
    keep = idx >= 0
    run = torch.zeros(idx.numel() + 1, dtype=torch.int64, device=idx.device)
    torch.cumsum(keep, 0, out=run[1:])
    return run[off.to(idx.device)], idx[keep].contiguous()


class IdentifierMap:
    """Identifier -> candidate position, -1 for identifiers the index does not
    hold.  Integer identifiers (a torch tensor): a sorted copy + searchsorted
    on their device.  String identifiers: libtt's host StringLookup
    (tt_vocab_*: row - 1, out of vocabulary -> -1), values compared as their
    str() text.  Identifiers are expected to be distinct; a repeated one maps
    to one of its positions."""

    def __init__(self, identifiers):
        self.n = len(identifiers)
        if isinstance(identifiers, torch.Tensor):
            if identifiers.is_floating_point():
                raise TypeError("identifiers must be integers or strings")
            self._sorted, self._order = torch.sort(identifiers.reshape(-1), stable=True)
            self._vocab = None
        else:
            from pkg.schema.vocab import NativeVocab

            self._vocab = NativeVocab(np.asarray(identifiers).reshape(-1))

    def positions(self, values) -> torch.Tensor:
        """int32 positions of `values` (flattened)."""
        if self._vocab is not None:
            if isinstance(values, torch.Tensor):
                values = values.cpu().numpy()
            if not isinstance(values, np.ndarray):
                values = list(values)
            if len(values) == 0:
                return torch.zeros(0, dtype=torch.int32)
            return torch.as_tensor(self._vocab.encode(values) - 1)
        v = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values, dtype=np.int64))
        v = v.reshape(-1).to(self._sorted.device, self._sorted.dtype)
        if self.n == 0 or v.numel() == 0:
            return torch.full((v.numel(),), -1, dtype=torch.int32, device=v.device)
        at = torch.searchsorted(self._sorted, v).clamp_(max=self.n - 1)
        hit = self._sorted[at] == v
        return torch.where(hit, self._order[at], torch.full_like(at, -1)).to(torch.int32)


def positions_of(identifiers, values) -> torch.Tensor:
    """Candidate positions (int32, -1 for unknown) of `values` among
    `identifiers`.  An index keeps the IdentifierMap it builds on first use."""
    return IdentifierMap(identifiers).positions(values)


def identifier_csr(id_map: IdentifierMap, exclusions, n_queries: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-query exclusions given as IDENTIFIERS -> the (off, idx) pair of
    their candidate positions; identifiers the index does not hold are
    dropped.  Accepted: a sequence of n_queries per-query sequences, a
    [n_queries, E] array / tensor (every entry an identifier; pad with one the
    index does not hold), or an (off, values) tuple."""
    n = int(n_queries)
    if isinstance(exclusions, tuple) and len(exclusions) == 2 and _is_array(exclusions[0]):
        off = _as_tensor(exclusions[0], torch.int64).reshape(-1).cpu()
        flat = exclusions[1]
    elif _is_array(exclusions) and exclusions.ndim == 2:
        if exclusions.shape[0] != n:
            raise ValueError(f"need one row of exclusions per query ({n}), got {exclusions.shape[0]}")
        off = torch.arange(n + 1, dtype=torch.int64) * int(exclusions.shape[1])
        flat = exclusions.reshape(-1)
    else:
        rows = [list(r.reshape(-1).tolist()) if _is_array(r) else list(r) for r in exclusions]
        if len(rows) != n:
            raise ValueError(f"need one exclusion list per query ({n}), got {len(rows)}")
        off = _offsets(torch.as_tensor([len(r) for r in rows], dtype=torch.int64).reshape(-1))
        flat = [v for r in rows for v in r]
    pos = id_map.positions(flat)
    if off.numel() != n + 1 or int(off[0]) != 0 or int(off[-1]) != pos.numel() or bool((off[1:] < off[:-1]).any()):
        raise ValueError("exclusion offsets must be [n_queries + 1], start at 0, be non-decreasing and end at "
                         "len(values)")
    return drop_negative(off, pos)


def run_classes(queries: torch.Tensor, k: int, n_candidates: int, exclusions,
                run: Callable[[torch.Tensor, int, torch.Tensor, torch.Tensor, int], Tuple[torch.Tensor, torch.Tensor]],
                k_max: int = K_LIMIT) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores [Q, k], indices [Q, k]) of `queries` [Q, E] without each
    query's `exclusions` (as_csr forms).  Per class of plan_classes,
    run(class queries, k', class off, class idx, class count) returns that
    class's ([Qc, k], [Qc, k]): the search at k' and, for count > 0, the
    filter to k.  A batch of one class runs on the whole batch as it is.  The
    plan is made, and its errors raised, before anything is launched."""
    Q = int(queries.shape[0])
    off, idx, counts = as_csr(exclusions, Q)
    classes = plan_classes(counts, k, n_candidates, k_max)
    dev = queries.device
    off, idx = off.to(dev), idx.to(dev)
    if len(classes) == 1:
        c = classes[0]
        return run(queries, c.k_search, off, idx, c.count)
    out_s = torch.empty(Q, k, dtype=torch.float32, device=dev)
    out_i = torch.empty(Q, k, dtype=torch.int32, device=dev)
    for c in classes:
        rows = c.rows.to(dev)
        coff, cidx = take_rows(off, idx, rows, c.total)
        s, i = run(queries.index_select(0, rows).contiguous(), c.k_search, coff, cidx, c.count)
        out_s[rows] = s
        out_i[rows] = i
    return out_s, out_i
