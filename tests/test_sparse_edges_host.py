"""CPU checks behind tests/test_sparse_edges_gpu.py and test_gather_tagged_gpu.py.

The GPU tests compare libtt with oracle/ bit for bit on the constructed cases
of tests/sparse_cases.py.  That proves something only if (a) the oracle
itself is right, checked here against an independent numpy loop, and (b) the
inputs are sensitive to the summation order, so that a kernel adding in
another order, or sorting unstably, cannot produce the same bits.  The host
side of the entry points (argument validation: clean errors, no launch) is
checked through the C ABI as tests/test_native_exports.py does.
"""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import sparse_cases as sc
from oracle import oracle
from pkg import _native

CHUNK = oracle.GPU_DEDUP_CHUNK


def test_block_constants_match_the_kernel_source():
    src = open(os.path.join(os.path.dirname(_native.__file__), "..", "..", "csrc", "tt_sparse.hip")).read()
    assert int(re.search(r"constexpr int kBlock = (\d+);", src).group(1)) == sc.BLOCK == CHUNK
    assert int(re.search(r"constexpr int kPFJoin = (\d+);", src).group(1)) == sc.PF_JOIN


def test_ids_from_counts_places_runs():
    rng = np.random.default_rng(0)
    counts = [3, 0, 40, 1]
    ids = sc.ids_from_counts(counts, 6, rng, num_rows=9)
    assert ids.dtype == np.int32 and len(ids) == 50
    valid = ids[(ids >= 0) & (ids < 9)]
    assert np.array_equal(np.bincount(valid, minlength=4), counts)
    assert set(ids[(ids < 0) | (ids >= 9)]) <= {-1, -7, 9, 14}
    assert not np.array_equal(valid, np.sort(valid))  # shuffled
    assert sc.run_spans(counts) == [(0, 0, 3), (2, 3, 43), (3, 43, 44)]
    assert sc.piece_sizes(3, 43) == [29, 11] and sc.piece_sizes(31, 33) == [1, 1]


def test_case_geometry_is_what_the_table_says():
    """Each constructed case places its boundaries where its comment in
    sparse_cases.py says."""
    g = sc.GEOMETRY
    assert all(b % 32 == 0 and e - b == 32 for _, b, e in sc.run_spans(g["A"].counts))
    assert sc.order_kind(g["A"].counts) == "block"
    spans = sc.run_spans(g["B"].counts)
    assert [e - b for _, b, e in spans][:5] == [31, 2, 30, 2, 30]
    assert all(sc.piece_sizes(b, e) == [1, 1] for _, b, e in spans[1::2])
    assert sc.order_kind(g["B"].counts) == "flat"
    assert sc.run_spans(g["C"].counts)[:2] == [(3, 0, 64), (10, 64, 129)]
    for k in (1, 32, 33, 34):
        row, b, e = sc.run_spans(g[f"D{k}"].counts)[31]
        assert (b, e) == (31, 32 + 32 * k) and len(sc.piece_sizes(b, e)) == k + 1
    for name, n_mod in (("E", 0), ("F", 5)):
        row, b, e = sc.run_spans(g[name].counts)[-1]
        assert len(sc.piece_sizes(b, e)) == 3 and e == g[name].counts.sum() and g[name].batch % 32 == n_mod
    assert g["E"].n_invalid == 0 and g["E"].batch == g["E"].counts.sum()
    assert g["F"].n_invalid == 40
    assert sc.run_spans(g["G"].counts) == [(1234, 0, 4096)]
    assert g["H"].counts.sum() == 0 and g["H"].n_invalid == 200
    c0, c1 = sc.CASE_I_COUNTS
    assert sc.run_spans(c0)[-1] == (7, 30, 96) and sc.run_spans(c1)[0] == (7, 0, 70)
    assert c0.sum() == c1.sum() == 96
    assert sorted(n for n in g if g[n].star) == ["C", "D1", "D32", "D33", "D34", "G"]


def _host_cases():
    """(label, rows, ids, grad, counts) of every constructed single-table case."""
    out = []
    for dim in sc.GEOM_DIMS:
        for name in sc.GEOMETRY_NAMES:
            c = sc.GEOMETRY[name]
            out.append((f"{name}-d{dim}", sc.GEOM_ROWS, c.ids(), c.grad(dim), c.counts))
        ids, grad = sc.case_i_inputs(dim)
        for t in range(2):
            out.append((f"I{t}-d{dim}", sc.CASE_I_ROWS[t], ids[t], grad[:, t * dim:(t + 1) * dim], sc.CASE_I_COUNTS[t]))
        for rows in sc.CASE_J_ROWS:
            ids = sc.case_j_ids(rows)
            valid = ids[(ids >= 0) & (ids < rows)]
            out.append((f"J{rows}-d{dim}", rows, ids, sc.wide_grad(np.random.default_rng(rows), len(ids), dim),
                        np.bincount(valid, minlength=rows)))
        for b in sc.CASE_K_BATCHES[1:]:
            ids = sc.case_k_ids(b)
            valid = ids[(ids >= 0) & (ids < sc.CASE_K_ROWS)]
            out.append((f"K{b}-d{dim}", sc.CASE_K_ROWS, ids, sc.wide_grad(np.random.default_rng(b), b, dim),
                        np.bincount(valid, minlength=sc.CASE_K_ROWS)))
    return out


HOST_CASES = _host_cases()


def _valid(ids, grad, rows):
    ok = (ids >= 0) & (ids < rows)
    return ids[ok], np.ascontiguousarray(grad[ok])


@pytest.mark.parametrize("label,rows,ids,grad,counts", HOST_CASES, ids=[c[0] for c in HOST_CASES])
def test_oracle_against_independent_loop(label, rows, ids, grad, counts):
    """The C oracle in the GPU's blocked order against a plain numpy loop in
    TF's flat order: bit-identical wherever the two orders coincide (runs
    inside one block, or later pieces of one lookup), otherwise within the
    fp32 summation bound 2 * count * 2^-24 * sum|g| of test_dedup_sum_bitexact."""
    vi, vg = _valid(ids, grad, rows)
    u_naive, s_naive = sc.naive_scatter_sum(ids, grad, rows)
    u_blk, s_blk = oracle.dedup_sum(vi, vg, chunk=CHUNK)
    u_flat, s_flat = oracle.dedup_sum(vi, vg, chunk=0)
    assert np.array_equal(u_naive, np.flatnonzero(counts))
    assert np.array_equal(u_blk, u_naive) and np.array_equal(u_flat, u_naive)
    assert np.array_equal(s_flat, s_naive)  # the oracle's flat order is the independent loop's
    u_nb, s_nb = sc.naive_blocked_sum(ids, grad, rows)
    assert np.array_equal(u_nb, u_naive) and np.array_equal(s_blk, s_nb)  # and its blocked order, on every case
    kind = sc.order_kind(counts)
    if kind in ("block", "flat"):
        assert np.array_equal(s_blk, s_naive)
    else:
        _, s_abs = sc.naive_scatter_sum(ids, np.abs(grad), rows)
        bound = 2.0 * counts[u_naive].astype(np.float64)[:, None] * 2.0 ** -24 * s_abs.astype(np.float64)
        assert np.all(np.abs(s_blk.astype(np.float64) - s_naive.astype(np.float64)) <= bound + 1e-30)


LONG_CASES = [c for c in HOST_CASES if sc.order_kind(c[4]) == "long"]


def test_long_cases_cover_the_table():
    names = {c[0].split("-")[0] for c in LONG_CASES}
    assert {"C", "D1", "D32", "D33", "D34", "E", "F", "G", "I0", "I1"} <= names
    assert any(n.startswith("J") for n in names)


@pytest.mark.parametrize("label,rows,ids,grad,counts", LONG_CASES, ids=[c[0] for c in LONG_CASES])
def test_long_cases_are_order_sensitive(label, rows, ids, grad, counts):
    """A bit-exact GPU comparison can fail only if the inputs notice the order:
    the blocked sum differs from the flat one, and reversing the lookups'
    batch order (what an unstable sort may do) changes a summed element."""
    vi, vg = _valid(ids, grad, rows)
    _, s_blk = oracle.dedup_sum(vi, vg, chunk=CHUNK)
    _, s_flat = oracle.dedup_sum(vi, vg, chunk=0)
    assert not np.array_equal(s_blk, s_flat)
    _, s_rev = oracle.dedup_sum(vi[::-1], vg[::-1], chunk=CHUNK)
    assert not np.array_equal(s_blk, s_rev)
    # a run of three or more pieces: the order in which the join adds the
    # later pieces shows too
    if any(len(sc.piece_sizes(b, e)) >= 3 for _, b, e in sc.run_spans(counts)):
        _, s_swapped = sc.naive_blocked_sum(ids, grad, rows, later_pieces_reversed=True)
        assert not np.array_equal(s_blk, s_swapped)


@pytest.mark.parametrize("step", sc.EXACT_STEPS)
def test_adam_exact_beta_powers(step):
    """beta1 = 1/2, beta2 = 3/4: every power used is a fp32 number, and the
    oracle's powf returns exactly that number."""
    b1, b2 = sc.EXACT_BETAS
    b1p, b2p = oracle.adam_powers(b1, b2, step)
    for beta, got in ((b1, b1p), (b2, b2p)):
        exact = Fraction(beta) ** step
        assert Fraction(float(np.float32(float(exact)))) == exact  # representable
        assert got.dtype == np.float32 and Fraction(float(got)) == exact


# --------------------------------------------------------------------------- host validation
FAKE = 4096  # a non-NULL, 16-byte aligned address no call below dereferences


def _table(num_rows=100, dim=8, num_sources=1):
    t = (_native.SparseTable * 1)()
    _fill(t[0], num_rows, dim, num_sources)
    return t


def _fill(t, num_rows, dim, num_sources):
    t.table, t.slot0, t.slot1 = FAKE, FAKE, FAKE
    t.num_rows, t.dim, t.num_sources = num_rows, dim, num_sources
    for s in range(min(num_sources, _native.MAX_SOURCES)):
        t.ids[s] = FAKE
        t.grad_col_offset[s] = 0


def _raises(rc, code, *words):
    assert rc == code
    with pytest.raises(_native.TTError) as e:
        _native.check(rc)
    msg = str(e.value)
    assert all(w in msg for w in words), msg


def _adagrad(t, n):
    return _native.lib().tt_sparse_adagrad(t, n, 4, FAKE, 64, 0.05, 1e-7, FAKE, 1 << 40, None)


def _adam(t, n):
    return _native.lib().tt_sparse_adam(t, n, 4, FAKE, 64, 1e-3, 0.5, 0.75, 1e-7, 1, FAKE, 1 << 40, None)


def _scatter(t, n):
    return _native.lib().tt_sparse_scatter_sum(t, n, 4, FAKE, 64, FAKE, 1 << 40, None)


@pytest.mark.parametrize("entry", [_adagrad, _adam, _scatter], ids=["adagrad", "adam", "scatter_sum"])
def test_sparse_entries_reject_bad_tables(entry):
    _raises(entry(_table(dim=0), 1), _native.TT_ERR_BAD_ARG, "dim=0")
    _raises(entry(_table(dim=4097), 1), _native.TT_ERR_BAD_ARG, "dim=4097")
    _raises(entry(_table(num_sources=5), 1), _native.TT_ERR_BAD_ARG, "num_sources=5")
    _raises(entry(_table(num_rows=2 ** 30), 1), _native.TT_ERR_BAD_ARG, "num_rows")


def test_dedup_rejects_bad_dim():
    L = _native.lib()
    for dim in (0, 4097):
        rc = L.tt_dedup_sum(FAKE, 10, 100, FAKE, 8, dim, FAKE, FAKE, FAKE, FAKE, 1 << 40, None)
        _raises(rc, _native.TT_ERR_BAD_ARG, f"dim={dim}")
    rc = L.tt_dedup_sum(FAKE, 10, 2 ** 30, FAKE, 8, 8, FAKE, FAKE, FAKE, FAKE, 1 << 40, None)
    _raises(rc, _native.TT_ERR_BAD_ARG, "num_rows")


def test_dense_adagrad_many_rejects_nine_jobs():
    jobs = (_native.DenseJob * 9)()
    for j in jobs:
        j.param, j.accum, j.grad, j.n = FAKE, FAKE, FAKE, 4
    _raises(_native.lib().tt_dense_adagrad_many(jobs, 9, 0.05, 1e-7, None), _native.TT_ERR_BAD_ARG, "jobs", "9")
    _raises(_native.lib().tt_dense_adagrad_many(jobs, 0, 0.05, 1e-7, None), _native.TT_ERR_BAD_ARG, "jobs")


def test_sparse_sort_takes_at_most_16_tables():
    t = (_native.SparseTable * 17)()
    for x in t:
        _fill(x, 100, 8, 1)
    rc = _native.lib().tt_sparse_sort(t, 17, 4, FAKE, 1 << 40, None)
    _raises(rc, _native.TT_ERR_BAD_ARG, "at most 16 tables")


def test_keys_wider_than_32_bits_are_unsupported():
    """16 tables of 2^29 rows: 4 table bits + 30 id bits."""
    t = (_native.SparseTable * 16)()
    for x in t:
        _fill(x, 2 ** 29, 8, 1)
    assert _native.lib().tt_sparse_workspace_size(t, 16, 4) == 0
    _raises(_adagrad(t, 16), _native.TT_ERR_UNSUPPORTED, "32-bit keys")
    _raises(_scatter(t, 16), _native.TT_ERR_UNSUPPORTED, "32-bit keys")


def test_empty_gradient_is_row_major():
    """B = 0: numpy hands an empty [0, W] array over with zero strides; the
    wrappers take it (nothing is read) and still refuse a transposed one."""
    import torch

    from pkg.modelling import hip_ops

    empty = torch.as_tensor(np.zeros((0, 5), np.float32))
    assert hip_ops._row_major(empty, "grad") == 5
    assert hip_ops._row_major(torch.zeros(4, 7)[:, 2:5], "grad") == 7
    with pytest.raises(ValueError):
        hip_ops._row_major(torch.zeros(5, 4).t(), "grad")


def _max_tagged():
    src = open(os.path.join(os.path.dirname(_native.__file__), "..", "..", "csrc", "tt_gather.hip")).read()
    return int(re.search(r"constexpr int kMaxTagged = (\d+);", src).group(1))


def _tagged(num_tables=1, dim=8, out=FAKE, out_stride=None, table=FAKE):
    t = (_native.RowTable * num_tables)()
    for x in t:
        x.table, x.num_rows = table, 7
    stride = dim + 4 if out_stride is None else out_stride
    return _native.lib().tt_gather_tagged(t, num_tables, dim, FAKE, FAKE, 1, out, stride, None)


def test_gather_tagged_rejects_bad_shapes():
    _raises(_tagged(dim=6), _native.TT_ERR_BAD_ARG, "dim=6")
    _raises(_tagged(dim=1028), _native.TT_ERR_BAD_ARG, "dim=1028")
    _raises(_tagged(dim=0), _native.TT_ERR_BAD_ARG, "dim=0")
    _raises(_tagged(out=FAKE + 4), _native.TT_ERR_BAD_ARG, "16-byte aligned")
    _raises(_tagged(out_stride=10), _native.TT_ERR_BAD_ARG, "16-byte aligned")
    _raises(_tagged(out_stride=4), _native.TT_ERR_BAD_ARG, "16-byte aligned")   # narrower than dim
    _raises(_tagged(table=FAKE + 8), _native.TT_ERR_BAD_ARG, "table 0")
    _raises(_tagged(num_tables=_max_tagged() + 1), _native.TT_ERR_BAD_ARG, f"1..{_max_tagged()} tables")
