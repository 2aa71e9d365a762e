"""CPU: the brute-force index's host plan, and that the edge cases bite.

* tt_bruteforce_lds_bytes (the dynamic LDS a search asks of one workgroup)
  fits the 160 KiB of a CU for every k the search accepts; up to k = 1120 it
  equals the formulas of the code before the fallback's large-k forms,
  restated in tests/index_cases.py; the workspace sizes up to that k equal
  the values recorded from that code (tests/golden/index_plan_parent.json).
  The restated 4-wave formula itself passes the limit at k = 1121 and at all
  but 14 of the k above: what the library asked for on every such search
  before.
* every constructed input of tests/index_cases.py has, on the oracle alone,
  the property its GPU test (tests/test_index_edges_gpu.py) relies on.
"""
import json
import os

import numpy as np
import pytest

import index_cases as ic
from oracle import oracle
from pkg import _native

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_plan_parent.json")


def _tie_group(q_row, c, k):
    """(k-th score, (k+1)-th score, number of candidates scoring the k-th) of one query."""
    s = oracle.fmaf_scores(q_row[None, :], c)[0]
    top = np.sort(s)[::-1]
    return top[k - 1], top[k], int(np.count_nonzero(s == top[k - 1]))


# ---- the plan ---------------------------------------------------------------
def test_lds_requests_fit_for_every_k():
    lib = _native.lib()
    for k in range(1, ic.K_MAX + 1):
        fin, fb = lib.tt_bruteforce_lds_bytes(k, 0), lib.tt_bruteforce_lds_bytes(k, 1)
        assert 0 < fin <= ic.LDS_LIMIT, (k, fin)
        assert 0 < fb <= ic.LDS_LIMIT, (k, fb)
    for k, which in [(0, 0), (ic.K_MAX + 1, 1), (100, 2), (100, -1)]:
        assert lib.tt_bruteforce_lds_bytes(k, which) == 0


def test_lds_requests_unchanged_up_to_1120():
    lib = _native.lib()
    for k in range(1, ic.K_PARENT_FITS + 1):
        assert lib.tt_bruteforce_lds_bytes(k, 0) == ic.final_lds_bytes(k), k
        assert lib.tt_bruteforce_lds_bytes(k, 1) == ic.fallback_lds_bytes(k), k


def test_restated_formulas_reproduce_the_known_values():
    """The restatement against figures worked out by hand from the source,
    and the reason for the large-k forms: the 4-wave request passes the limit
    at k = 1121."""
    assert [ic.fallback_lds_bytes(k) for k in (1000, 1024, 1100, 1121, 2048, 4000)] == \
        [150592, 152128, 162528, 165752, 225856, 429632]
    assert [ic.final_lds_bytes(k) for k in (1000, 1024, 1100, 1121, 2048, 4000)] == \
        [30768, 31280, 50224, 50736, 76336, 147504]
    assert all(ic.fallback_lds_bytes(k) <= ic.LDS_LIMIT for k in range(1, ic.K_PARENT_FITS + 1))
    # parts drops from 7 to 6 at k = 1171, which lets 1171..1184 fit once more; nothing above does
    over = [k for k in range(1, ic.K_MAX + 1) if ic.fallback_lds_bytes(k) > ic.LDS_LIMIT]
    assert over == list(range(1121, 1171)) + list(range(1185, ic.K_MAX + 1))
    assert ic.fallback_lds_bytes(4000, waves=1, parts=1) == 132416


def test_large_k_fallback_requests_are_a_restated_form():
    """Above 1120 the request is the same formula on fewer waves, then fewer
    parts: the most waves of (4, 2, 1) that fit with the plan's parts, else
    one wave with the most parts that fit."""
    lib = _native.lib()
    for k in range(ic.K_PARENT_FITS + 1, ic.K_MAX + 1):
        parts = ic.plan(k).parts
        forms = [(w, parts) for w in (4, 2, 1)] + [(1, p) for p in range(parts - 1, 0, -1)]
        want = next(ic.fallback_lds_bytes(k, w, p) for w, p in forms if ic.fallback_lds_bytes(k, w, p) <= ic.LDS_LIMIT)
        assert lib.tt_bruteforce_lds_bytes(k, 1) == want, k


def test_workspace_sizes_unchanged_up_to_1120():
    lib = _native.lib()
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert len(golden["sizes"]) == 3
    for key, vals in golden["sizes"].items():
        nq, n, dim = (int(v) for v in key.split("x"))
        assert len(vals) == ic.K_PARENT_FITS
        got = [int(lib.tt_bruteforce_workspace_size(nq, n, dim, k)) for k in range(1, ic.K_PARENT_FITS + 1)]
        assert got == vals, key


# ---- the cases bite ---------------------------------------------------------
def test_large_k_cases_cross_the_named_thresholds():
    ks = sorted({k for _, k in ic.LARGE_K})
    assert ks == [1001, 1024, 1025, 1121, 2048, 2049, 4000]
    assert ic.plan(1024).P == ic.ALIAS_P and ic.plan(1025).P == 2048
    assert ic.plan(2048).P == 2048 and ic.plan(2049).P == 4096
    assert ic.fallback_lds_bytes(1120) <= ic.LDS_LIMIT < ic.fallback_lds_bytes(1121)
    assert (4000, 4000) in ic.LARGE_K
    for n, k in ic.LARGE_K:
        for signed in (False, True):
            q, c = ic.large_k(n, k, signed)
            assert q.shape == (70, 32) and c.shape == (n, 32) and k <= n
            assert not q[ic.LARGE_K_ZERO_ROW].any() and (c.min() < 0) == signed and (q.min() < 0) == signed
            assert not q.flags.writeable and not c.flags.writeable


@pytest.mark.parametrize("k", ic.FALLBACK_K)
def test_large_k_fallback_tie_group_is_longer_than_the_staged_list(k):
    q, c = ic.fallback_large_k(k)
    T = ic.fallback_ties(k)
    assert c.shape[0] == T + 1500 and q.shape[0] == 8
    kth, nxt, group = _tie_group(q[ic.FALLBACK_TIE_QUERY], c, k)
    assert kth == nxt
    assert group >= T > ic.plan(k).LF
    _, ri = ic.expected(("fallback_large_k", k), k)
    assert np.array_equal(ri[ic.FALLBACK_TIE_QUERY], ic.FALLBACK_TIE_ROW0 + np.arange(k))


def test_mass_fallback_every_query_ties_past_the_staged_list():
    q, c = ic.mass_fallback()
    assert q.shape == (1100, 32) and q.shape[0] > ic.FB_SLOTS and len(np.unique(q, axis=0)) == 1100
    assert ic.plan(ic.MASS_K).LF == 1024
    s = oracle.fmaf_scores(q, c)
    kth = np.sort(s, axis=1)[:, -ic.MASS_K]
    assert ((s == kth[:, None]).sum(axis=1) > 1024).all()
    _, ri = ic.expected(("mass_fallback",), ic.MASS_K)
    assert np.array_equal(ri, np.broadcast_to(ic.MASS_TIES[0] + np.arange(ic.MASS_K), ri.shape))


def test_odd_dims_cross_the_padded_widths():
    assert [d for d in ic.ODD_DIMS if d % 4 == 0] == []
    pads = [32 if d <= 32 else 64 if d <= 64 else 128 for d in ic.ODD_DIMS]
    assert pads == [32, 32, 32, 64, 64, 128, 128]
    assert ic.OFFSET_DIM % 4 == 0 and ic.OFFSET_PITCH % 4 == 0
    for n, _ in ic.ODD_SHAPES:
        q, c = ic.odd_dim(33, n)
        assert (c.min() < 0) == (n == 700) and (q.min() < 0) == (n == 700)


def test_mixed_modes_every_run_of_32_holds_every_kind():
    for has_neg in (False, True):
        q, c = ic.mixed_modes(has_neg)
        assert (c.min() < 0) == has_neg and int((c < 0).sum()) == (1 if has_neg else 0)
        for r0 in range(0, ic.MIXED_Q - 31, 32):
            kinds = set()
            for i in range(r0, r0 + 32):
                row = q[i]
                if (row < 0).any():
                    kinds.add(ic.KIND_SIGNED)
                elif not row.any():
                    kinds.add(ic.KIND_NEG_ZERO if np.signbit(row).all() else ic.KIND_ZERO)
                    assert np.signbit(row).all() or not np.signbit(row).any()
                elif np.signbit(row).sum() == 1 and (row[~np.signbit(row)] > 0).all():
                    kinds.add(ic.KIND_ONE_NEG_ZERO)
                else:
                    assert not np.signbit(row).any()
                    kinds.add(ic.KIND_NONNEG)
            assert kinds == {ic.KIND_SIGNED, ic.KIND_ZERO, ic.KIND_NEG_ZERO, ic.KIND_ONE_NEG_ZERO, ic.KIND_NONNEG}, r0
        assert ic.MIXED_Q // 32 == 4


@pytest.mark.parametrize("kind", ic.ORDERED_KINDS)
def test_ordered_topk_sits_at_one_end(kind):
    q, c = ic.ordered(kind)
    n, k = ic.ORDERED_N, ic.ORDERED_K
    assert c.shape == (n, 32) and n % ic.TILE == 3 and q.shape == (64, 32)
    _, ri = ic.expected(("ordered", kind), k)
    srt = np.sort(ri, axis=1)
    if kind == "ascending":
        assert np.array_equal(srt, np.broadcast_to(np.arange(n - k, n), srt.shape))
    elif kind == "descending":
        assert np.array_equal(srt, np.broadcast_to(np.arange(k), srt.shape))
    else:
        assert np.array_equal(srt[:, -ic.ORDERED_TAIL:], np.broadcast_to(np.arange(n - ic.ORDERED_TAIL, n),
                                                                         (64, ic.ORDERED_TAIL)))
        assert (srt[:, :-ic.ORDERED_TAIL] < n - ic.ORDERED_TAIL).all()
        # and they out-score everything else: the first 35 of every answer
        assert (ri[:, :ic.ORDERED_TAIL] >= n - ic.ORDERED_TAIL).all()


def test_exclusion_rows_reach_the_long_class():
    from pkg.modelling.indices import exclusions

    q, c = ic.exclusion_problem()
    rows = ic.exclusion_rows()
    assert c.shape[0] == 3001 and len(rows) == q.shape[0]
    long_row = rows[ic.EXCL_LONG_QUERY]
    assert len(long_row) == len(set(long_row)) == 1200 > 1024
    _, top, _ = oracle.bruteforce_topk(q, c, ic.EXCL_POOL)
    assert set(long_row) <= set(top[ic.EXCL_LONG_QUERY].tolist())
    assert ic.EXCL_K + len(long_row) == 1300 <= exclusions.K_LIMIT
    assert ic.fallback_lds_bytes(1300) > ic.LDS_LIMIT
