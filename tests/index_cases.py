"""Constructed inputs for the brute-force index's edge tests (no GPU needed).

The index (csrc/tt_index.hip) promises the exact top-k of the fp32 fmaf-chain
scores (score descending, index ascending) for dim <= 128 and k <= 4000.
Which code answers a query depends on k (the sort size P = next_pow2(k), the
finalize's staged list LF, the fallback's per-wave list L and its parts), on
the layout of the rows (float4 or scalar rescoring), on the signs of the data
(relative or absolute screen bound per query) and on whether the finalize can
certify the query's screened list at all (else: the exact fallback).  The
cases here are built to reach each of those, and every case's expected answer
is oracle.bruteforce_topk(q, c, k), compared with np.array_equal.

The arrays are deterministic, built once per process and read-only.
tests/test_index_edges_host.py checks on the CPU that each case bites (the
conditions named with the builders below) and the host plan (LDS bytes,
workspace sizes); tests/test_index_edges_gpu.py runs the cases through libtt.
"""
import functools
from typing import List, NamedTuple, Tuple

import numpy as np

from oracle import oracle

LDS_LIMIT = 163840     # bytes of LDS one workgroup can have (160 KiB per CU)
K_MAX = 4000           # tt_bruteforce_search's largest k
K_PARENT_FITS = 1120   # largest k whose 4-wave fallback fits LDS_LIMIT
ALIAS_P = 1024         # kAliasP: largest sort size whose keys alias the finalize's list
FB_SLOTS = 1024        # kFbSlots: failed queries per chunk served part by part
FB_WAVES = 4           # kFbWaves
LF_MIN = 1024          # TT_INDEX_LF
TILE = 64              # kCTile


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def next_pow2(x: int) -> int:
    p = 1
    while p < x:
        p *= 2
    return p


class Plan(NamedTuple):
    """What plan_search derives from k alone."""
    L: int       # the fallback's per-wave list
    LF: int      # the finalize's staged list
    P: int       # bitonic sort size
    parts: int   # candidate parts per failed query
    NW: int      # waves per finalize workgroup


def plan(k: int) -> Plan:
    L = round_up(2 * k + 256, 64)
    LF = max(L, LF_MIN)
    NW = 4 if k >= 512 else 1
    if NW > 1:
        LF = max(LF, round_up(int(3.5 * k) + 128, 64))
    return Plan(L, LF, next_pow2(max(k, 2)), min(max(8192 // k, 1), 64), NW)


def final_lds_bytes(k: int) -> int:
    """final_lds_bytes(LF, P, NW): query row, (score, id) list, the ranking keys
    when they cannot alias the list, 256 radix bins, 2 NW + 4 aux words."""
    p = plan(k)
    return 512 + p.LF * 8 + (0 if p.P <= ALIAS_P else p.P * 8) + 1024 + (2 * p.NW + 4) * 4


def fallback_lds_bytes(k: int, waves: int = FB_WAVES, parts: int = 0) -> int:
    """fallback_lds_bytes: query row, per wave a list of L and 256 bins, the
    merge buffer of max(parts, waves) * k entries, P sort keys, 16 words.
    With the defaults: the 4-wave form with the plan's parts, the only one
    before the large-k forms existed."""
    p = plan(k)
    parts = parts or p.parts
    return 512 + waves * (p.L * 8 + 1024) + max(parts, waves) * k * 8 + p.P * 8 + 64


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _relu(rng, shape, scale=1.0):
    return np.maximum(rng.standard_normal(shape) * scale, 0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def expected(case: Tuple, k: int):
    """(scores, indices) of the oracle for a case key (name, *args) below."""
    q, c = CASES[case[0]](*case[1:])
    s, i, _ = oracle.bruteforce_topk(q, c, k)
    return _ro(s, i)


# ---- 1. large k -------------------------------------------------------------
# 1001: first k above what the suite ran before; 1025: first P > kAliasP (the
# ranking keys leave the list's LDS); 1121: first k whose 4-wave fallback
# passes the LDS limit; 2049: first P = 4096; (4000, 4000): k == n_cand.
LARGE_K = [(5000, 1001), (5000, 1024), (5000, 1025), (5000, 1121), (6000, 2048), (6000, 2049), (9000, 4000),
           (4000, 4000)]
LARGE_K_E, LARGE_K_Q, LARGE_K_ZERO_ROW = 32, 70, 3


@functools.lru_cache(maxsize=None)
def large_k(n: int, k: int, signed: bool):
    rng = np.random.default_rng(7000 + 31 * n + k + (1 if signed else 0))
    c = rng.standard_normal((n, LARGE_K_E)).astype(np.float32)
    q = rng.standard_normal((LARGE_K_Q, LARGE_K_E)).astype(np.float32)
    if not signed:
        c, q = np.maximum(c, 0), np.maximum(q, 0)
    q[LARGE_K_ZERO_ROW] = 0
    return _ro(q, c)


# ---- 2. large-k fallback ----------------------------------------------------
# T identical rows 3 * base and one query equal to base: its T best scores are
# one tie group, longer than the finalize's staged list LF.  The finalize
# cannot cut such a query in LDS.  Either its tau sits at or above the tied
# screen score (the ties are unlisted, the list is short of k or the
# certificate fails) or all T ties are listed: ntot > LF (not staged), the
# k-th screened score is the tied one, every tie passes ub >= X and the kept
# count passes L.  Both ends are `fail`: the query goes to the fallback, whose
# answer must be the k lowest tied indices in order.
FALLBACK_K = [1121, 2048, 4000]
FALLBACK_E, FALLBACK_Q, FALLBACK_TIE_QUERY, FALLBACK_TIE_ROW0 = 32, 8, 5, 500


def fallback_ties(k: int) -> int:
    return round_up(int(3.5 * k) + 128, 64) + 512


@functools.lru_cache(maxsize=None)
def fallback_large_k(k: int):
    rng = np.random.default_rng(8000 + k)
    T = fallback_ties(k)
    base = _relu(rng, FALLBACK_E)
    c = _relu(rng, (T + 1500, FALLBACK_E), 0.1)
    c[FALLBACK_TIE_ROW0:FALLBACK_TIE_ROW0 + T] = base * np.float32(3.0)
    q = _relu(rng, (FALLBACK_Q, FALLBACK_E))
    q[FALLBACK_TIE_QUERY] = base
    return _ro(q, c)


# ---- 3. more than kFbSlots failed queries in one chunk ----------------------
# every query is a positive multiple of base, so each one's best 2000 scores
# tie: 1100 failures, 1024 served part by part and 76 scanned whole.
MASS_N, MASS_E, MASS_K, MASS_Q, MASS_TIES = 3000, 32, 100, 1100, (500, 2500)


@functools.lru_cache(maxsize=None)
def mass_fallback():
    rng = np.random.default_rng(8100)
    base = _relu(rng, MASS_E) + np.float32(0.125)
    c = _relu(rng, (MASS_N, MASS_E), 0.1)
    c[MASS_TIES[0]:MASS_TIES[1]] = base * np.float32(3.0)
    scales = (0.5 + np.arange(MASS_Q) / 256.0).astype(np.float32)  # distinct, exact in fp32
    q = (scales[:, None] * base[None, :]).astype(np.float32)
    return _ro(q, c)


# ---- 4. scalar rescoring and padded dims ------------------------------------
# dims across both pick_dpad boundaries (32 | 33, 64 | 65), none a multiple
# of 4 except through the layouts below; (700, 20) keeps every score of a
# split, (3000, 100) samples.
ODD_DIMS = [1, 3, 30, 33, 50, 65, 127]
ODD_SHAPES = [(700, 20), (3000, 100)]
ODD_Q = 45
OFFSET_DIM, OFFSET_PITCH = 32, 36   # float4-shaped rows whose base is one float past an aligned address


@functools.lru_cache(maxsize=None)
def odd_dim(dim: int, n: int):
    """Signed rows at n = 700, non-negative ones at n = 3000."""
    rng = np.random.default_rng(8200 + 131 * dim + n)
    c = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((ODD_Q, dim)).astype(np.float32)
    if n != 700:
        c, q = np.maximum(c, 0) + np.float32(0.01), np.maximum(q, 0) + np.float32(0.01)
    return _ro(q, c)


# ---- 5. mixed bound modes ---------------------------------------------------
# kinds by position inside each run of 32 queries (one MFMA query set)
MIXED_Q, MIXED_N, MIXED_E, MIXED_KS = 130, 5000, 64, (1, 100)
KIND_SIGNED, KIND_ZERO, KIND_NEG_ZERO, KIND_ONE_NEG_ZERO, KIND_NONNEG = "signed", "+0", "-0", "one -0", "nonneg"
_MIXED_SLOTS = {1: KIND_SIGNED, 9: KIND_SIGNED, 20: KIND_SIGNED, 5: KIND_ZERO, 13: KIND_NEG_ZERO,
                27: KIND_ONE_NEG_ZERO}


def mixed_kind(i: int) -> str:
    return _MIXED_SLOTS.get(i % 32, KIND_NONNEG)


@functools.lru_cache(maxsize=None)
def mixed_modes(has_neg: bool):
    """Non-negative candidates and queries of every kind in each run of 32;
    has_neg: row 1234 holds one negative coordinate, which makes every
    query's bound absolute."""
    rng = np.random.default_rng(8300)
    c = _relu(rng, (MIXED_N, MIXED_E))
    if has_neg:
        c[1234, 17] = np.float32(-0.25)
    q = np.empty((MIXED_Q, MIXED_E), np.float32)
    for i in range(MIXED_Q):
        kind = mixed_kind(i)
        if kind == KIND_SIGNED:
            q[i] = rng.standard_normal(MIXED_E)
        elif kind == KIND_ZERO:
            q[i] = 0.0
        elif kind == KIND_NEG_ZERO:
            q[i] = -0.0
        elif kind == KIND_ONE_NEG_ZERO:
            q[i] = np.abs(rng.standard_normal(MIXED_E)) + 0.01
            q[i, 40] = -0.0
        else:
            q[i] = np.maximum(rng.standard_normal(MIXED_E), 0)
    return _ro(q, c)


# ---- 6. ordered candidates --------------------------------------------------
# 40003 = 625 * 64 + 3: the last tile holds 3 rows.  "tail": the last 35 rows
# (that partial tile and half of the full tile before it) out-score the rest.
ORDERED_N, ORDERED_E, ORDERED_Q, ORDERED_K, ORDERED_TAIL = 40003, 32, 64, 100, 35
ORDERED_KINDS = ["ascending", "descending", "tail"]


@functools.lru_cache(maxsize=None)
def ordered(kind: str):
    rng = np.random.default_rng(8400)
    d = (np.abs(rng.standard_normal(ORDERED_E)) + 0.5).astype(np.float32)  # the dominant direction
    c = _relu(rng, (ORDERED_N, ORDERED_E))
    scales = (0.5 + np.arange(ORDERED_Q) / 64.0).astype(np.float32)
    q = (scales[:, None] * d[None, :]).astype(np.float32)
    if kind == "tail":
        c[-ORDERED_TAIL:] += np.float32(4.0) * d
    else:
        order = np.argsort(c.astype(np.float64) @ d.astype(np.float64), kind="stable")
        c = np.ascontiguousarray(c[order] if kind == "ascending" else c[order[::-1]])
    return _ro(q, c)


# ---- 7. product paths -------------------------------------------------------
EXCL_N, EXCL_E, EXCL_K, EXCL_Q, EXCL_LONG_QUERY, EXCL_LONG, EXCL_POOL = 3001, 32, 100, 6, 2, 1200, 1300
SHARD_CASE = ("large_k", 6000, 2048, False)
SHARD_K = 2048


@functools.lru_cache(maxsize=None)
def exclusion_problem():
    rng = np.random.default_rng(8500)
    c = _relu(rng, (EXCL_N, EXCL_E))
    q = _relu(rng, (EXCL_Q, EXCL_E))
    return _ro(q, c)


@functools.lru_cache(maxsize=None)
def exclusion_rows() -> Tuple[Tuple[int, ...], ...]:
    """Per query the excluded candidates: query EXCL_LONG_QUERY drops 1200 of
    its own best 1300 (the "more than 1024 exclusions" class, searched at
    k' = 1300); the others none, or five of their best ten."""
    q, c = exclusion_problem()
    _, top, _ = oracle.bruteforce_topk(q, c, EXCL_POOL)
    rng = np.random.default_rng(8501)
    rows: List[Tuple[int, ...]] = []
    for i in range(EXCL_Q):
        if i == EXCL_LONG_QUERY:
            rows.append(tuple(int(v) for v in rng.permutation(top[i])[:EXCL_LONG]))
        elif i % 2:
            rows.append(tuple(int(v) for v in top[i, :10:2]))
        else:
            rows.append(())
    return tuple(rows)


CASES = {"large_k": large_k, "fallback_large_k": fallback_large_k, "mass_fallback": mass_fallback,
         "odd_dim": odd_dim, "mixed_modes": mixed_modes, "ordered": ordered}
