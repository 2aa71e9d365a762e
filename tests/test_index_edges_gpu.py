"""GPU: the brute-force index where its suite had not been: k in (1000, 4000],
dims that are no multiple of 4 and unaligned rows, more failed queries than
the fallback has slots, mixed per-query bound modes, ordered candidates.

Inputs: tests/index_cases.py (tests/test_index_edges_host.py shows on the CPU
that each one reaches what it is named for).  Every expected answer is
oracle.bruteforce_topk and every comparison is np.array_equal on indices and
on scores: no tolerances.
"""
import numpy as np
import pytest
import torch

import index_cases as ic
import topk_exclude_ref as ref
from oracle import oracle
from pkg import _native
from pkg.modelling import hip_ops
from pkg.modelling.indices.brute_force import BruteForceIndex

pytestmark = pytest.mark.gpu


def _t(x, dev):
    return torch.as_tensor(np.array(x), device=dev)  # a copy: the cases are read-only


def _search(dev, q, c, k):
    tc = _t(c, dev)
    s, i = hip_ops.bruteforce_search(hip_ops.bruteforce_build(tc), tc, _t(q, dev), k)
    return s.cpu().numpy(), i.cpu().numpy()


def _check(dev, case, k):
    q, c = ic.CASES[case[0]](*case[1:])
    s, i = _search(dev, q, c, k)
    rs, ri = ic.expected(case, k)
    assert np.array_equal(i, ri)
    assert np.array_equal(s, rs)


# ---- 1. large k -------------------------------------------------------------
@pytest.mark.parametrize("signed", [False, True], ids=["relu", "signed"])
@pytest.mark.parametrize("n,k", ic.LARGE_K)
def test_large_k(cuda, n, k, signed):
    _check(cuda, ("large_k", n, k, signed), k)


def test_k_4001_still_raises(cuda):
    q, c = ic.large_k(9000, 4000, False)
    with pytest.raises(_native.TTError, match="4000"):
        _search(cuda, q, c, ic.K_MAX + 1)


_OVER_BUDGET = """
import sys
import numpy as np, torch
from pkg import _native
from pkg.modelling import hip_ops
dev = torch.device("cuda:0")
c = torch.as_tensor(np.random.default_rng(0).standard_normal((700, 32)).astype(np.float32), device=dev)
try:
    hip_ops.bruteforce_search(hip_ops.bruteforce_build(c), c, c[:8], 20)
except _native.TTError as e:
    torch.cuda.synchronize()
    print("TTERROR", e)
    sys.exit(0)
sys.exit("the search went through")
"""


def test_over_budget_lds_request_is_a_message_not_a_launch(cuda):
    """TT_FINAL_LF (read once per process, hence the child) stages 20,032
    entries: 512 + 20032 * 8 + 1024 + 24 = 161,816 B fits, 20,352 entries do
    not (164,376 B).  The search must return an error naming k and the bytes
    before it sets the kernel's attribute or launches it."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TT_FINAL_LF="20352",
               PYTHONPATH=os.pathsep.join([root, os.path.join(root, "hm-retrieval-two-tower_amd")]))
    r = subprocess.run([sys.executable, "-c", _OVER_BUDGET], env=env, cwd=root, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TTERROR" in r.stdout and "k=20 " in r.stdout and "164376" in r.stdout, r.stdout


# ---- 2. large-k fallback ----------------------------------------------------
@pytest.mark.parametrize("k", ic.FALLBACK_K)
def test_large_k_fallback(cuda, k):
    _check(cuda, ("fallback_large_k", k), k)


# ---- 3. more than 1024 failed queries in a chunk ----------------------------
def test_mass_fallback_whole_query_form(cuda):
    _check(cuda, ("mass_fallback",), ic.MASS_K)


# ---- 4. scalar rescoring and padded dims ------------------------------------
def _pitched(x, dev, pitch, offset=0):
    """x as a [:, :dim] view of a NaN-filled buffer with row pitch `pitch`
    whose first element sits `offset` floats into the allocation."""
    n, dim = x.shape
    flat = torch.full((n * pitch + offset,), float("nan"), device=dev)
    view = flat[offset:offset + n * pitch].view(n, pitch)[:, :dim]
    view.copy_(_t(x, dev))
    assert view.stride() == (pitch, 1) and view.data_ptr() == flat.data_ptr() + 4 * offset
    return view


def _search_views(tq, tc, k):
    s, i = hip_ops.bruteforce_search(hip_ops.bruteforce_build(tc), tc, tq, k)
    return s.cpu().numpy(), i.cpu().numpy()


@pytest.mark.parametrize("layout", ["contiguous", "pitch+1"])
@pytest.mark.parametrize("n,k", ic.ODD_SHAPES)
@pytest.mark.parametrize("dim", ic.ODD_DIMS)
def test_odd_dims(cuda, dim, n, k, layout):
    q, c = ic.odd_dim(dim, n)
    if layout == "contiguous":
        tq, tc = _t(q, cuda), _t(c, cuda)
    else:
        tq, tc = _pitched(q, cuda, dim + 1), _pitched(c, cuda, dim + 1)
    s, i = _search_views(tq, tc, k)
    rs, ri = ic.expected(("odd_dim", dim, n), k)
    assert np.array_equal(i, ri)
    assert np.array_equal(s, rs)


@pytest.mark.parametrize("n,k", ic.ODD_SHAPES)
def test_float4_shaped_rows_off_alignment(cuda, n, k):
    """dim 32 and a pitch of 36: float4-shaped, but the base is one float past
    a 16-byte boundary, so the rescoring must not load float4."""
    q, c = ic.odd_dim(ic.OFFSET_DIM, n)
    tq, tc = _pitched(q, cuda, ic.OFFSET_PITCH, 1), _pitched(c, cuda, ic.OFFSET_PITCH, 1)
    assert tc.data_ptr() % 16 == 4
    s, i = _search_views(tq, tc, k)
    rs, ri = ic.expected(("odd_dim", ic.OFFSET_DIM, n), k)
    assert np.array_equal(i, ri)
    assert np.array_equal(s, rs)


# ---- 5. mixed bound modes ---------------------------------------------------
@pytest.mark.parametrize("has_neg", [False, True], ids=["nonneg-candidates", "one-negative-coordinate"])
@pytest.mark.parametrize("k", ic.MIXED_KS)
def test_mixed_bound_modes(cuda, k, has_neg):
    _check(cuda, ("mixed_modes", has_neg), k)


# ---- 6. ordered candidates --------------------------------------------------
@pytest.mark.parametrize("kind", ic.ORDERED_KINDS)
def test_ordered_candidates(cuda, kind):
    _check(cuda, ("ordered", kind), ic.ORDERED_K)


# ---- 7. through the product paths -------------------------------------------
def test_search_with_1200_exclusions(cuda):
    q, c = ic.exclusion_problem()
    rows = [list(r) for r in ic.exclusion_rows()]
    rs, ri = ref.filtered_topk(oracle.fmaf_scores(q, c), rows, ic.EXCL_K)
    index = BruteForceIndex(ic.EXCL_K, None, [(torch.arange(ic.EXCL_N, dtype=torch.int32), torch.tensor(c))],
                            device=cuda)
    s, i = index.search(_t(q, cuda), exclusions=rows)
    assert np.array_equal(i.cpu().numpy(), ri)
    assert np.array_equal(s.cpu().numpy(), rs)


def test_shard_search_world_1_equals_search(cuda):
    q, c = ic.CASES[ic.SHARD_CASE[0]](*ic.SHARD_CASE[1:])
    tc, tq = _t(c, cuda), _t(q, cuda)
    index = hip_ops.bruteforce_build(tc)
    s, i = hip_ops.bruteforce_search(index, tc, tq, ic.SHARD_K)
    ss, si = hip_ops.bruteforce_shard_search(index, tc, tq, ic.SHARD_K, 0, lambda t: None)
    assert torch.equal(si, i)
    assert torch.equal(ss.view(torch.int32), s.view(torch.int32))
    rs, ri = ic.expected(ic.SHARD_CASE, ic.SHARD_K)
    assert np.array_equal(i.cpu().numpy(), ri) and np.array_equal(s.cpu().numpy(), rs)
