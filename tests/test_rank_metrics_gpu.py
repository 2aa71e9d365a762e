"""GPU: tt_rank_metrics against the numpy restatement (tests/rank_metrics_ref.py).

vals (as int32 bit patterns), hits and m are bit-equal to the restatement; the
accumulators are bit-equal to the restated 256-lane reduction and within 1e-12
relative of math.fsum.  Shapes cover both launch forms (one wave per query up
to k_list = 256 and T = 64, one workgroup per query above), list lengths
around the 64-position words of the hit bitmap, 1 / 5 / 257 queries (a ragged
last workgroup of the four-queries-per-workgroup form), strided rows, and ks
unsorted and repeated.  Every case holds every kind of row.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import rank_metrics_ref as ref
from pkg import _native
from pkg.modelling import hip_ops

PAD = ref.PAD
SMALL_K, SMALL_T = 256, 64  # the one-wave-per-query form's limits (kRankSmallK, kRankSmallT)
K_LISTS = [1, 12, 63, 64, 65, SMALL_K, SMALL_K + 1, 1000, 4096]
TS = [1, 5, SMALL_T, SMALL_T + 1, 1024]
NQ = 257
KINDS = 8


def _ks(k_list):
    """Unsorted, repeated, with k = 1 and k = k_list."""
    return [k_list, 1, min(12, k_list), k_list, max(1, k_list // 2), 1, min(65, k_list)]


def _fit(values, n, fill=-1):
    out = np.full(n, fill, np.int64)
    values = np.asarray(values, np.int64)[:n]
    out[:values.size] = values
    return out


@functools.lru_cache(maxsize=None)
def _case(k_list, T):
    """(cand [257, k_list], truth [257, T], ks, restated vals / hits / m) —
    row q is of kind q % 8; computed once, shared, never modified."""
    rng = np.random.default_rng(100000 * T + k_list)
    cand = np.empty((NQ, k_list), np.int64)
    truth = np.empty((NQ, T), np.int64)
    universe = max(4, 2 * max(k_list, T))
    for q in range(NQ):
        kind = q % KINDS
        c = rng.integers(0, universe, k_list)  # a small universe: repeats and hits are frequent
        t = rng.integers(0, universe, T)
        if kind == 0:    # padding in the middle of the truth row, repeats on both sides
            t[rng.random(T) < 0.4] = -1
        elif kind == 1:  # no truth at all
            t = rng.choice([-1, PAD, -2 ** 31, -7], T)
        elif kind == 2:  # PAD and negative truth ids among valid ones; the list ends in a PAD tail
            t[::3] = PAD
            t[1::3] = -t[1::3] - 1
            c[k_list - k_list // 3:] = PAD
            c[rng.random(k_list) < 0.1] = -1
        elif kind == 3:  # the list repeats three ids over and over
            c = rng.choice(t[:3] if T >= 3 else np.concatenate([t, [universe + 1, universe + 2]]), k_list)
        elif kind == 4:  # every position a hit while the truth lasts (m >= k_list when T >= k_list)
            ids = rng.permutation(universe)[:max(k_list, T)]
            c, t = _fit(ids, k_list), rng.permutation(_fit(ids, T))
        elif kind == 5:  # ids congruent modulo 4096: long probe chains for a low-bits hash
            c = 7 + 4096 * rng.integers(0, min(universe, 2 ** 19), k_list)
            t = 7 + 4096 * rng.integers(0, min(universe, 2 ** 19), T)
        elif kind == 6:  # valid truth, none of it in the list
            t = t + universe
        else:            # one distinct true id, T times
            t[:] = c[rng.integers(k_list)] if q % 16 == 7 else universe + 5
        cand[q], truth[q] = c, t
    cand, truth = cand.astype(np.int32), truth.astype(np.int32)
    ks = _ks(k_list)
    vals, hits, m = ref.rank_metrics(cand, truth, ks)
    for a in (cand, truth, vals, hits, m):
        a.setflags(write=False)
    return cand, truth, ks, vals, hits, m


def test_cases_reach_every_kind_of_row():
    """On the restatement alone: the parametrised cases hold unscored rows,
    full-hit rows with m >= k_list, rows with no hit, repeated list entries
    that are credited once, PAD tails, and both launch forms."""
    full = unscored = no_hit = repeats = tails = 0
    forms = set()
    for k_list in K_LISTS:
        for T in TS:
            cand, truth, ks, vals, hits, m = _case(k_list, T)
            forms.add(k_list <= SMALL_K and T <= SMALL_T)
            full += int(((m >= k_list) & (hits[:, 0] == k_list)).sum())
            unscored += int((m == 0).sum())
            no_hit += int(((m > 0) & (hits[:, 0] == 0)).sum())
            tails += int((cand[:, -1] == PAD).sum())
            q = 3  # kind 3: three ids repeated; at most three hits however long the list
            repeats += int(hits[q, 0] <= 3 < k_list and m[q] >= 1)
            assert ks[0] == k_list and 1 in ks and len(ks) != len(set(ks)) and (k_list == 1 or ks != sorted(ks))
    assert forms == {True, False}
    assert full >= 5 and unscored >= 45 and no_hit >= 45 and repeats >= 10 and tails >= 10


def _acc(dev, nk):
    return (torch.zeros(nk, 4, dtype=torch.float64, device=dev), torch.zeros(nk, 2, dtype=torch.int64, device=dev),
            torch.zeros(1, dtype=torch.int64, device=dev))


def _same(got, want):
    vals, hits, m = (x.cpu().numpy() for x in got)
    rv, rh, rm = want
    assert np.array_equal(m, rm)
    assert np.array_equal(hits, rh)
    assert np.array_equal(vals.view(np.int32), rv.view(np.int32))


def _same_acc(acc, want):
    f64, i64, nv = (x.cpu().numpy() for x in acc)
    assert np.array_equal(nv, want[2]) and np.array_equal(i64, want[1])
    assert np.array_equal(f64.view(np.int64), want[0].view(np.int64)), (f64, want[0])


@pytest.mark.gpu
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("k_list", K_LISTS)
def test_rank_metrics_matches_the_restatement(cuda, k_list, T):
    cand, truth, ks, rv, rh, rm = _case(k_list, T)
    nk = len(ks)
    # strided rows (ld_cand > k_list, ld_truth > T); the columns past the row would all be hits if read
    wide_c = torch.full((NQ, k_list + 3), int(truth[0, 0]) if truth[0, 0] >= 0 else 1, dtype=torch.int32, device=cuda)
    wide_t = torch.arange(T + 5, dtype=torch.int32, device=cuda).repeat(NQ, 1)
    wide_c[:, :k_list] = torch.tensor(cand, device=cuda)
    wide_t[:, :T] = torch.tensor(truth, device=cuda)
    tc, tt_ = wide_c[:, :k_list], wide_t[:, :T]
    acc = _acc(cuda, nk)
    got = hip_ops.rank_metrics(tc, tt_, ks, acc)
    assert got[0].shape == (NQ, nk, 4) and got[0].dtype == torch.float32
    assert got[1].shape == (NQ, nk) and got[1].dtype == torch.int32 and got[2].dtype == torch.int32
    _same(got, (rv, rh, rm))
    want1 = ref.reduce_acc(rv, rh, rm)
    _same_acc(acc, want1)
    scored = rm > 0
    for j in range(nk):
        for c in range(4):
            exact = math.fsum(float(v) for v in rv[scored, j, c])
            assert abs(float(acc[0][j, c]) - exact) <= 1e-12 * abs(exact)
    # the same call again: identical bits, and a fresh accumulator holds the same sums
    acc_b = _acc(cuda, nk)
    again = hip_ops.rank_metrics(tc, tt_, ks, acc_b)
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _same_acc(acc_b, want1)
    # 5 queries and 1 query (contiguous rows, another kind of row per case), accumulated on top of the 257
    s5 = (k_list + T) % (NQ - 5)
    s1 = (3 * k_list + T) % NQ
    want = want1
    for s, n in ((s5, 5), (s1, 1)):
        sub = hip_ops.rank_metrics(torch.tensor(cand[s:s + n], device=cuda),
                                   torch.tensor(truth[s:s + n], device=cuda), ks, acc)
        _same(sub, (rv[s:s + n], rh[s:s + n], rm[s:s + n]))
        want = ref.reduce_acc(rv[s:s + n], rh[s:s + n], rm[s:s + n], want)
    _same_acc(acc, want)
    # the first 63 queries of the 257-query call are a 63-query call; no accumulators: one launch
    first = hip_ops.rank_metrics(tc[:63], tt_[:63], ks)
    for a, b in zip(first, got):
        assert torch.equal(a.view(torch.int32), b[:63].view(torch.int32))
    # the inputs were only read
    assert np.array_equal(tc.cpu().numpy(), cand) and np.array_equal(tt_.cpu().numpy(), truth)


@pytest.mark.gpu
def test_c_entry_without_m_out_and_a_truth_vector(cuda):
    """The C ABI with m_out = NULL (with and without accumulators), and
    hip_ops with a [Q] truth vector (T = 1)."""
    cand, truth, ks, rv, rh, rm = _case(12, 5)
    tc, tt_ = torch.tensor(cand, device=cuda), torch.tensor(truth, device=cuda)
    disc, idcg = (torch.tensor(a, device=cuda) for a in ref.tables(12))
    nk = len(ks)
    ks_arr = (ctypes.c_int32 * nk)(*ks)
    for with_acc in (False, True):
        vals = torch.full((NQ, nk, 4), -1.0, device=cuda)
        hits = torch.full((NQ, nk), -1, dtype=torch.int32, device=cuda)
        acc = _acc(cuda, nk)
        ptrs = [a.data_ptr() for a in acc] if with_acc else [None] * 3
        _native.check(_native.lib().tt_rank_metrics(tc.data_ptr(), 12, 12, tt_.data_ptr(), 5, 5, NQ, ks_arr, nk,
                                                    disc.data_ptr(), idcg.data_ptr(), vals.data_ptr(),
                                                    hits.data_ptr(), None, *ptrs,
                                                    torch.cuda.current_stream().cuda_stream))
        assert np.array_equal(vals.cpu().numpy().view(np.int32), rv.view(np.int32))
        assert np.array_equal(hits.cpu().numpy(), rh)
        if with_acc:
            _same_acc(acc, ref.reduce_acc(rv, rh, rm))
    cand1, truth1, ks1, rv1, rh1, rm1 = _case(65, 1)
    got = hip_ops.rank_metrics(torch.tensor(cand1, device=cuda), torch.tensor(truth1[:, 0].copy(), device=cuda),
                               ks1)
    _same(got, (rv1, rh1, rm1))
    with pytest.raises(ValueError):
        hip_ops.rank_metrics(tc, tt_, [13])
    with pytest.raises(TypeError):
        hip_ops.rank_metrics(tc.long(), tt_, [1])
