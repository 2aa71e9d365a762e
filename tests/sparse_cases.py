"""Constructed inputs for the embedding-update tests (no GPU needed).

The sparse update (csrc/tt_sparse.hip) sorts each table's lookups by row id,
cuts the sorted list into aligned blocks of BLOCK lookups, sums every
segment's piece of a block sequentially and joins the pieces of segments that
span blocks.  Which branch a segment takes depends on where it starts and
ends relative to the blocks, so the cases here are given as COUNTS per row
id: after the stable sort row i occupies the sorted positions
[sum(counts[:i]), sum(counts[:i + 1])), invalid ids sort behind every valid
one, and the caller decides exactly where the boundaries fall.

tests/test_sparse_edges_host.py checks the cases themselves on the CPU (the
oracle against an independent loop, and that the inputs are sensitive to the
summation order); tests/test_sparse_edges_gpu.py runs them through libtt.
"""
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

BLOCK = 32     # kBlock: sorted lookups per summation block
PF_JOIN = 32   # kPFJoin: pieces loaded per batch by the join
GEOM_ROWS = 4096
GEOM_DIMS = (8, 100)   # P = 8 (8 blocks per wave, divergent end search); P = 64 with a ragged column trip


def ids_from_counts(counts, n_invalid: int, rng: np.random.Generator, num_rows: Optional[int] = None) -> np.ndarray:
    """int32 ids in which id i occurs counts[i] times, plus n_invalid ids from
    {-1, -7, num_rows, num_rows + 5} (num_rows: len(counts) unless given),
    shuffled by a permutation drawn from rng."""
    counts = np.asarray(counts, dtype=np.int64)
    rows = len(counts) if num_rows is None else int(num_rows)
    assert len(counts) <= rows and np.all(counts >= 0)
    valid = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    pool = np.array([-1, -7, rows, rows + 5], dtype=np.int64)
    invalid = pool[rng.integers(0, len(pool), size=n_invalid)]
    ids = np.concatenate([valid, invalid])
    return ids[rng.permutation(len(ids))].astype(np.int32)


def wide_grad(rng: np.random.Generator, n: int, w: int) -> np.ndarray:
    """fp32 [n, w] normal values scaled by 2^-8 .. 2^8 per element: every fp32
    sum of a few of them depends on its order, so a wrong summation order or
    an unstable sort changes bits."""
    scale = 2.0 ** rng.integers(-8, 9, size=(n, w))
    return (rng.standard_normal((n, w)) * scale).astype(np.float32)


def naive_scatter_sum(ids: np.ndarray, grad: np.ndarray, rows: int) -> Tuple[np.ndarray, np.ndarray]:
    """(distinct valid ids ascending, their gradient sums): per id the rows are
    added in increasing batch position starting from fp32 0 (TF's flat
    UnsortedSegmentSum order, no chunking).  Plain numpy, independent of
    oracle/tt_oracle.c."""
    ids = np.asarray(ids).reshape(-1)
    grad = np.asarray(grad, dtype=np.float32)
    uniq = sorted({int(i) for i in ids if 0 <= int(i) < rows})
    sums = np.zeros((len(uniq), grad.shape[1]), np.float32)
    for u, row in enumerate(uniq):
        acc = np.zeros(grad.shape[1], np.float32)
        for p in np.flatnonzero(ids == row):  # increasing batch position
            acc = acc + grad[p]
        sums[u] = acc
    return np.asarray(uniq, np.int32), sums


def naive_blocked_sum(ids: np.ndarray, grad: np.ndarray, rows: int,
                      later_pieces_reversed: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The GPU's order in plain numpy: the valid lookups sorted stably by id are
    cut into aligned blocks of BLOCK; each run's piece of a block is summed
    sequentially from 0 and the pieces are added in order starting from 0.
    later_pieces_reversed: the pieces after a run's first added last to first
    (what a join with a wrong loop order would compute)."""
    ids = np.asarray(ids).reshape(-1)
    grad = np.asarray(grad, dtype=np.float32)
    uniq = np.asarray(sorted({int(i) for i in ids if 0 <= int(i) < rows}), np.int32)
    sums = np.zeros((len(uniq), grad.shape[1]), np.float32)
    begin = 0  # sorted position of the current row's first lookup
    for u, row in enumerate(uniq):
        pos = np.flatnonzero(ids == row)
        pieces, k = [], 0
        for size in piece_sizes(begin, begin + len(pos)):
            acc = np.zeros(grad.shape[1], np.float32)
            for p in pos[k:k + size]:
                acc = acc + grad[p]
            pieces.append(acc)
            k += size
        if later_pieces_reversed:
            pieces = pieces[:1] + pieces[:0:-1]
        out = np.zeros(grad.shape[1], np.float32)
        for piece in pieces:
            out = out + piece
        sums[u] = out
        begin += len(pos)
    return uniq, sums


def counts_of(num_rows: int, runs: List[Tuple[int, int]]) -> np.ndarray:
    """counts[num_rows] from (row, count) pairs listed in increasing row order."""
    rows = [r for r, _ in runs]
    assert rows == sorted(set(rows)) and rows[-1] < num_rows
    counts = np.zeros(num_rows, np.int64)
    for r, c in runs:
        counts[r] = c
    return counts


def run_spans(counts) -> List[Tuple[int, int, int]]:
    """(row, first sorted position, end) of every row with lookups."""
    counts = np.asarray(counts, np.int64)
    ends = np.cumsum(counts)
    return [(int(r), int(ends[r] - counts[r]), int(ends[r])) for r in np.flatnonzero(counts)]


def piece_sizes(begin: int, end: int) -> List[int]:
    """Lookups of the sorted run [begin, end) in each aligned block it touches."""
    out = []
    while begin < end:
        nxt = min((begin // BLOCK + 1) * BLOCK, end)
        out.append(nxt - begin)
        begin = nxt
    return out


def order_kind(counts) -> str:
    """How the blocked summation order relates to the flat one for these counts:
    "block": every run lies inside one aligned block;
    "flat":  some run crosses a block edge, but every piece after a run's
             first holds one lookup: (0 + p1) + g == p1 + g, still the flat order;
    "long":  some later piece holds two or more lookups: the blocked sum
             associates differently and is only close to the flat one."""
    kind = "block"
    for _, b, e in run_spans(counts):
        pieces = piece_sizes(b, e)
        if len(pieces) > 1:
            kind = "flat" if kind == "block" else kind
            if max(pieces[1:]) > 1:
                kind = "long"
    return kind


class GeomCase(NamedTuple):
    name: str
    counts: np.ndarray   # per row id of a GEOM_ROWS-row table
    n_invalid: int
    star: bool           # also run through Adam and dedup_sum
    seed: int

    @property
    def batch(self) -> int:
        return int(self.counts.sum()) + self.n_invalid

    def ids(self) -> np.ndarray:
        return ids_from_counts(self.counts, self.n_invalid, np.random.default_rng(self.seed), GEOM_ROWS)

    def grad(self, dim: int) -> np.ndarray:
        return wide_grad(np.random.default_rng(1000 + self.seed), self.batch, dim)


def _case_d(k: int) -> np.ndarray:
    # 31 singles fill slots 0..30 of block 0; the run starts in slot 31 and
    # covers k whole blocks after it; a short tail follows
    runs = [(3 * i + 1, 1) for i in range(31)] + [(200, 1 + BLOCK * k), (300, 3), (4095, 2)]
    return counts_of(GEOM_ROWS, runs)


def _geometry_cases() -> Dict[str, GeomCase]:
    cases = [
        # A: every segment is exactly one block; no piece is ever written
        GeomCase("A", counts_of(GEOM_ROWS, [(5 * i + 1, BLOCK) for i in range(24)]), 0, False, 11),
        # B: 31, 2, 30, 2, 30, ...: every second segment straddles a block edge by one lookup
        GeomCase("B", counts_of(GEOM_ROWS, [(0, 31)] + [(2 + i, 2 if i % 2 == 0 else 30) for i in range(41)]), 3,
                 False, 12),
        # C: an aligned two-block run from sorted position 0 (seg_start = 0), then a
        # run of 65 from the next block edge, then a short one
        GeomCase("C", counts_of(GEOM_ROWS, [(3, 64), (10, 65), (11, 10)]), 5, True, 13),
        # E: n % 32 == 0, no invalid ids, the last run spans 3 blocks and ends at the region's end
        GeomCase("E", counts_of(GEOM_ROWS, [(i, 3) for i in range(10)] + [(4000, 66)]), 0, False, 15),
        # F: as E with n % 32 == 5 and 40 invalid ids: the invalid run spans blocks behind the joined run
        # (seed: at 16 the one joined run's 8 columns did not notice the order of its later pieces)
        GeomCase("F", counts_of(GEOM_ROWS, [(i, 3) for i in range(9)] + [(4000, 66)]), 40, False, 56),
        # G: every lookup one row: one join over 128 blocks
        GeomCase("G", counts_of(GEOM_ROWS, [(1234, 4096)]), 0, True, 17),
        # H: nothing valid
        GeomCase("H", np.zeros(GEOM_ROWS, np.int64), 200, False, 18),
    ]
    # D: the run starts in the last slot of a block (seg_start = 31); the join's
    # piece loop takes k pieces: one, exactly one batch of PF_JOIN, one and two more
    for k in (1, PF_JOIN, PF_JOIN + 1, PF_JOIN + 2):
        cases.append(GeomCase(f"D{k}", _case_d(k), 4, True, 140 + k))
    return {c.name: c for c in cases}


GEOMETRY = _geometry_cases()
GEOMETRY_NAMES = sorted(GEOMETRY)
STAR_NAMES = [n for n in GEOMETRY_NAMES if GEOMETRY[n].star]

# I: two tables in one call (one batch of 96 lookups each).  Table 0 ends with a
# 3-block run of row 7 at its region's end; table 1 begins with a 3-block run
# of row 7: the runs are neighbours in the sorted array and must not be joined.
CASE_I_ROWS = (GEOM_ROWS, 300)
CASE_I_COUNTS = (counts_of(CASE_I_ROWS[0], [(i, 5 if i < 2 else 4) for i in range(7)] + [(7, 66)]),
                 counts_of(CASE_I_ROWS[1], [(7, 70), (8, 20), (299, 6)]))
CASE_I_SEED = 19

# J: row counts at the edges of the sort key's id bits; ids include the last
# valid row and the first invalid one
CASE_J_ROWS = (255, 256, 1023, 1024)
CASE_J_BATCH = 300

# K: the smallest regions (3 rows)
CASE_K_BATCHES = (0, 1, 31, 32, 33)
CASE_K_ROWS = 3


def case_i_inputs(dim: int):
    """[(rows, ids, grad columns)] of case I's two tables and the shared gradient [96, 2 * dim]."""
    rng = np.random.default_rng(CASE_I_SEED)
    ids = [ids_from_counts(c, 0, rng, r) for c, r in zip(CASE_I_COUNTS, CASE_I_ROWS)]
    assert len(ids[0]) == len(ids[1])
    return ids, wide_grad(rng, len(ids[0]), 2 * dim)


def case_j_ids(num_rows: int) -> np.ndarray:
    rng = np.random.default_rng(num_rows)
    ids = ((rng.zipf(1.1, size=CASE_J_BATCH) - 1) % num_rows).astype(np.int32)
    ids[::7] = num_rows - 1   # the last valid row, many times: a run across blocks
    ids[3::11] = num_rows     # the first invalid id
    ids[5::53] = -1
    return ids


def case_k_ids(batch: int) -> np.ndarray:
    rng = np.random.default_rng(50 + batch)
    ids = rng.integers(0, CASE_K_ROWS, size=batch).astype(np.int32)
    if batch >= 31:
        ids[7] = CASE_K_ROWS  # one invalid lookup
    return ids


# Adam betas whose powers are exact in fp32 for every step used
EXACT_BETAS = (0.5, 0.75)
EXACT_STEPS = (1, 2, 3)
DEFAULT_BETAS = (0.9, 0.999)
