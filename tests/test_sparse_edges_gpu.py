"""The embedding update after its sort, at the shapes the Zipf tests never reach.

tests/test_kernels_gpu.py pins the sort stage of csrc/tt_sparse.hip; these
tests pin what follows it (block_sum_kernel, join_kernel, the applies, the
launch groups of 16 tables) and the dense optimizers beside it:

  dims       1 .. 300, odd and ragged against the 64-lane column loop, with a
             gradient buffer wider than the table at an odd column offset;
  tables     four sources per table; 17 and 33 tables in one call (the second
             and third launch group reusing one workspace and header);
  geometry   segment boundaries placed on purpose (tests/sparse_cases.py);
  Adam       table, m and v, bit-exact for betas whose powers are fp32 numbers;
  dense      grid-stride second trips, tt_dense_adagrad_many's job search.

Every comparison is np.array_equal against oracle/ (the same IEEE operations
in the same order).  The one exception: with the default betas (0.9, 0.999)
the table of an Adam update is compared at rtol 2e-6 / atol 1e-7, because
lr_t holds powf(beta, step), where libm's and numpy's powf may differ in the
last bit; m and v do not depend on it and stay bit-exact.
tests/test_sparse_edges_host.py checks on the CPU that the constructed
inputs are sensitive to the summation order and that the oracle agrees with
an independent loop.
"""
import numpy as np
import pytest
import torch

import sparse_cases as sc
from oracle import oracle
from pkg.modelling import hip_ops

pytestmark = pytest.mark.gpu

LR, EPS = 0.05, 1e-7
ADAM_LR = 1e-3


def _t(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x), device=dev)


def _zipf(rng, n, rows, invalid=0.03):
    ids = ((rng.zipf(1.1, size=n) - 1) % rows).astype(np.int32)
    bad = rng.random(n) < invalid
    ids[bad] = rng.choice(np.array([-1, -7, rows, rows + 5], np.int32), size=int(bad.sum()))
    return ids


def _tab(rows, dim, ids, offs):
    return dict(rows=rows, dim=dim, ids=list(ids), offs=list(offs))


def _lookups(tab, grad):
    """A table's lookups as the update sees them: its sources concatenated."""
    ids = np.concatenate(tab["ids"]) if tab["ids"] else np.zeros(0, np.int32)
    g = np.concatenate([grad[:, o:o + tab["dim"]] for o in tab["offs"]])
    return ids, np.ascontiguousarray(g)


def _ref_sums(tab, grad):
    ids, g = _lookups(tab, grad)
    ok = (ids >= 0) & (ids < tab["rows"])
    return oracle.dedup_sum(ids[ok], g[ok], chunk=oracle.GPU_DEDUP_CHUNK)


def _specs(cuda, tabs, B, state, slots):
    specs = []
    for tab, st in zip(tabs, state):
        for i in tab["ids"]:
            assert len(i) == B
        d = dict(table=st[0], ids=[_t(i, cuda) for i in tab["ids"]], grad_col_offset=tab["offs"])
        for name, s in zip(slots, st[1:]):
            d[name] = s
        specs.append(d)
    return specs


def run_adagrad(cuda, tabs, B, grad, seed=0):
    rng = np.random.default_rng(seed)
    w = [rng.uniform(-0.05, 0.05, (t["rows"], t["dim"])).astype(np.float32) for t in tabs]
    acc = [rng.uniform(0.05, 0.2, (t["rows"], t["dim"])).astype(np.float32) for t in tabs]
    state = [(_t(a, cuda), _t(b, cuda)) for a, b in zip(w, acc)]
    hip_ops.sparse_adagrad(_specs(cuda, tabs, B, state, ["slot0"]), B, _t(grad, cuda), LR, EPS)
    hip_ops.sparse_status(cuda)
    for i, tab in enumerate(tabs):
        ids, g = _lookups(tab, grad)
        oracle.sparse_adagrad(w[i], acc[i], ids, g, LR, EPS)
        assert np.array_equal(state[i][0].cpu().numpy(), w[i]), f"table {i}"
        assert np.array_equal(state[i][1].cpu().numpy(), acc[i]), f"accumulator {i}"


def run_scatter_sum(cuda, tabs, B, grad, seed=0):
    state = [(torch.zeros(t["rows"], t["dim"], device=cuda),) for t in tabs]
    hip_ops.sparse_scatter_sum(_specs(cuda, tabs, B, state, []), B, _t(grad, cuda))
    hip_ops.sparse_status(cuda)
    for i, tab in enumerate(tabs):
        ref = np.zeros((tab["rows"], tab["dim"]), np.float32)  # untouched rows stay zero
        uniq, sums = _ref_sums(tab, grad)
        ref[uniq] = sums
        assert np.array_equal(state[i][0].cpu().numpy(), ref), f"table {i}"


def adam_state(rng, tabs):
    """table, m, v with every element non-zero: rows no lookup touches still decay."""
    return [[rng.uniform(-0.05, 0.05, (t["rows"], t["dim"])).astype(np.float32),
             rng.uniform(-0.01, 0.01, (t["rows"], t["dim"])).astype(np.float32),
             rng.uniform(1e-5, 1e-3, (t["rows"], t["dim"])).astype(np.float32)] for t in tabs]


def run_adam(cuda, tabs, B, grad, seed=0, betas=sc.EXACT_BETAS, step=2):
    ref = adam_state(np.random.default_rng(seed), tabs)
    state = [tuple(_t(x, cuda) for x in r) for r in ref]
    hip_ops.sparse_adam(_specs(cuda, tabs, B, state, ["slot0", "slot1"]), B, _t(grad, cuda), ADAM_LR, betas[0],
                        betas[1], EPS, step)
    hip_ops.sparse_status(cuda)
    for i, tab in enumerate(tabs):
        ids, g = _lookups(tab, grad)
        oracle.sparse_adam(ref[i][0], ref[i][1], ref[i][2], ids, g, ADAM_LR, betas[0], betas[1], EPS, step)
        for got, want, name in zip(state[i], ref[i], ("table", "m", "v")):
            assert np.array_equal(got.cpu().numpy(), want), f"{name} {i}"


def run_dedup(cuda, tabs, B, grad, seed=0):
    (tab,) = tabs
    (ids,), (off,) = tab["ids"], tab["offs"]
    u_ref, s_ref = _ref_sums(tab, grad)
    u, s = hip_ops.dedup_sum(_t(ids, cuda), _t(grad, cuda)[:, off:off + tab["dim"]], tab["rows"])
    hip_ops.sparse_status(cuda, "dedup")
    assert np.array_equal(u.cpu().numpy(), u_ref)
    assert np.array_equal(s.cpu().numpy(), s_ref)


OPS = {"adagrad": run_adagrad, "scatter_sum": run_scatter_sum, "adam": run_adam, "dedup_sum": run_dedup}


# --------------------------------------------------------------------------- dims
@pytest.mark.parametrize("op", ["adagrad", "scatter_sum", "adam", "dedup_sum"])
@pytest.mark.parametrize("rows", [50, 5000])
@pytest.mark.parametrize("dim", [1, 2, 3, 5, 7, 33, 63, 65, 100, 129, 192, 300])
def test_dim_sweep(cuda, dim, rows, op):
    """Dims whose lanes idle (odd dim < 64), whose last column trip is ragged
    (65, 100, 129, 300) and above 128; 50 rows: long joined segments, 5000
    rows: mostly short ones; gradient rows wider than the table, read from
    column 3 (unaligned, row stride != dim)."""
    rng = np.random.default_rng(1000 * dim + rows)
    B = 1024
    ids = _zipf(rng, B, rows)
    grad = sc.wide_grad(rng, B, dim + 7)
    OPS[op](cuda, [_tab(rows, dim, [ids], [3])], B, grad, seed=dim)


@pytest.mark.parametrize("op", ["adagrad", "adam"])
@pytest.mark.parametrize("dim", [5, 130])
def test_four_sources(cuda, dim, op):
    """TT_MAX_SOURCES lookups of one table at column offsets 0, dim+1, 2dim+2,
    3dim+3 equal the oracle on the concatenated lookups."""
    rng = np.random.default_rng(dim)
    B, rows = 600, 300
    ids = [_zipf(rng, B, rows) for _ in range(4)]
    grad = sc.wide_grad(rng, B, 4 * dim + 4)
    OPS[op](cuda, [_tab(rows, dim, ids, [s * (dim + 1) for s in range(4)])], B, grad, seed=dim)


@pytest.mark.parametrize("op", ["adagrad", "adam", "scatter_sum"])
@pytest.mark.parametrize("num_tables", [17, 33])
def test_more_than_16_tables(cuda, num_tables, op):
    """One call over 17 and 33 tables: two and three launch groups, each
    sorting into and applying from the same workspace under its own header
    fingerprint.  Every table equals its own oracle run and no group records
    a status error."""
    rng = np.random.default_rng(num_tables)
    B = 512
    dims, rows = [1, 4, 6, 64, 130], [1, 40, 255, 256, 3000]
    tabs, off = [], 0
    for i in range(num_tables):
        d, r = dims[i % 5], rows[(i + i // 5) % 5]
        tabs.append(_tab(r, d, [_zipf(rng, B, r)], [off]))
        off += d
    grad = sc.wide_grad(rng, B, off + 1)
    OPS[op](cuda, tabs, B, grad, seed=num_tables)


# --------------------------------------------------------------------------- geometry
GEOM_PARAMS = [(n, d, op) for n in sc.GEOMETRY_NAMES for d in sc.GEOM_DIMS
               for op in (["adagrad", "scatter_sum"] + (["adam", "dedup_sum"] if sc.GEOMETRY[n].star else []))]


@pytest.mark.parametrize("name,dim,op", GEOM_PARAMS)
def test_segment_geometry(cuda, name, dim, op):
    """Cases A-H of tests/sparse_cases.py: segment starts and ends placed
    against the 32-lookup blocks, the region's end and the join's batches of
    32 pieces; dim 8 (8 blocks per wave: the end search's ballot under
    divergence) and dim 100 (64 lanes, ragged column trip)."""
    case = sc.GEOMETRY[name]
    OPS[op](cuda, [_tab(sc.GEOM_ROWS, dim, [case.ids()], [0])], case.batch, case.grad(dim), seed=case.seed)


@pytest.mark.parametrize("dim", sc.GEOM_DIMS)
def test_all_invalid_changes_nothing(cuda, dim):
    """Case H: with no valid lookup the table and accumulator keep every bit."""
    case = sc.GEOMETRY["H"]
    rng = np.random.default_rng(dim)
    w = rng.uniform(-0.05, 0.05, (sc.GEOM_ROWS, dim)).astype(np.float32)
    acc = rng.uniform(0.05, 0.2, (sc.GEOM_ROWS, dim)).astype(np.float32)
    tw, ta, ids, grad = _t(w, cuda), _t(acc, cuda), _t(case.ids(), cuda), _t(case.grad(dim), cuda)
    hip_ops.sparse_adagrad([dict(table=tw, slot0=ta, ids=[ids], grad_col_offset=[0])], case.batch, grad, LR, EPS)
    hip_ops.sparse_status(cuda)
    assert np.array_equal(tw.cpu().numpy(), w) and np.array_equal(ta.cpu().numpy(), acc)
    hip_ops.sparse_scatter_sum([dict(table=tw, ids=[ids], grad_col_offset=[0])], case.batch, grad)
    hip_ops.sparse_status(cuda)
    assert np.array_equal(tw.cpu().numpy(), w)


@pytest.mark.parametrize("op", ["adagrad", "scatter_sum"])
@pytest.mark.parametrize("dim", sc.GEOM_DIMS)
def test_runs_are_not_joined_across_tables(cuda, dim, op):
    """Case I: table 0's region ends with a 3-block run of row 7, table 1's
    begins with one."""
    ids, grad = sc.case_i_inputs(dim)
    tabs = [_tab(sc.CASE_I_ROWS[t], dim, [ids[t]], [t * dim]) for t in range(2)]
    OPS[op](cuda, tabs, len(ids[0]), grad, seed=sc.CASE_I_SEED)


@pytest.mark.parametrize("op", ["adagrad", "scatter_sum"])
@pytest.mark.parametrize("dim", sc.GEOM_DIMS)
@pytest.mark.parametrize("rows", sc.CASE_J_ROWS)
def test_last_row_and_first_invalid_id(cuda, rows, dim, op):
    """Case J: row counts on both sides of a power of two (the sort key's id
    bits and its invalid sentinel); row rows-1 is updated, id `rows` is not."""
    ids = sc.case_j_ids(rows)
    assert (ids == rows - 1).any() and (ids == rows).any()
    grad = sc.wide_grad(np.random.default_rng(rows), sc.CASE_J_BATCH, dim)
    OPS[op](cuda, [_tab(rows, dim, [ids], [0])], sc.CASE_J_BATCH, grad, seed=rows)


@pytest.mark.parametrize("op", ["adagrad", "scatter_sum"])
@pytest.mark.parametrize("dim", sc.GEOM_DIMS)
@pytest.mark.parametrize("B", sc.CASE_K_BATCHES)
def test_smallest_regions(cuda, B, dim, op):
    """Case K: regions of 0, 1, 31, 32 and 33 lookups on a 3-row table (B = 0
    returns cleanly; the oracle on no lookups changes nothing either)."""
    grad = sc.wide_grad(np.random.default_rng(B), B, dim)
    OPS[op](cuda, [_tab(sc.CASE_K_ROWS, dim, [sc.case_k_ids(B)], [0])], B, grad, seed=B)


# --------------------------------------------------------------------------- Adam
def _adam_tables(rng, B):
    """Two tables (dims 3 and 130), two sources each, ~3 % invalid ids."""
    shapes, tabs, off = [(200, 3), (1500, 130)], [], 0
    for rows, dim in shapes:
        tabs.append(_tab(rows, dim, [_zipf(rng, B, rows), _zipf(rng, B, rows)], [off, off + dim + 1]))
        off += 2 * dim + 2
    return tabs, off


def _adam_steps(cuda, betas):
    """Steps 1..3 with fresh ids and gradients: yields (gpu state, oracle state) after each."""
    rng = np.random.default_rng(7)
    B = 700
    tabs, width = _adam_tables(rng, B)
    ref = adam_state(rng, tabs)
    state = [tuple(_t(x, cuda) for x in r) for r in ref]
    for step in sc.EXACT_STEPS:
        for tab in tabs:
            tab["ids"] = [_zipf(rng, B, tab["rows"]) for _ in tab["ids"]]
        grad = sc.wide_grad(rng, B, width)
        hip_ops.sparse_adam(_specs(cuda, tabs, B, state, ["slot0", "slot1"]), B, _t(grad, cuda), ADAM_LR, betas[0],
                            betas[1], EPS, step)
        hip_ops.sparse_status(cuda)
        for i, tab in enumerate(tabs):
            ids, g = _lookups(tab, grad)
            oracle.sparse_adam(ref[i][0], ref[i][1], ref[i][2], ids, g, ADAM_LR, betas[0], betas[1], EPS, step)
        yield step, [[x.cpu().numpy() for x in s] for s in state], ref


def test_sparse_adam_exact_betas_bitexact(cuda):
    """beta1 = 0.5, beta2 = 0.75: beta^step is a fp32 number for steps 1..3, so
    lr_t is the same single-operation chain on both sides and table, m and v
    agree bit for bit, rows that only decay included."""
    for step, got, ref in _adam_steps(cuda, sc.EXACT_BETAS):
        for i in range(len(ref)):
            for g, r, name in zip(got[i], ref[i], ("table", "m", "v")):
                assert np.array_equal(g, r), f"step {step} {name} {i}"


def test_sparse_adam_default_betas(cuda):
    """beta1 = 0.9, beta2 = 0.999: only lr_t (through powf) may differ in its
    last bit, so table, m and v are compared at rtol 2e-6 / atol 1e-7; m and
    v do not depend on lr_t and must in addition be bit-exact."""
    for step, got, ref in _adam_steps(cuda, sc.DEFAULT_BETAS):
        for i in range(len(ref)):
            for g, r, name in zip(got[i], ref[i], ("table", "m", "v")):
                np.testing.assert_allclose(g, r, rtol=2e-6, atol=1e-7, err_msg=f"step {step} {name} {i}")
            assert np.array_equal(got[i][1], ref[i][1]), f"step {step} m {i}"
            assert np.array_equal(got[i][2], ref[i][2]), f"step {step} v {i}"


def _dense_adam(cuda, n, betas, steps, rng):
    p = rng.standard_normal(n).astype(np.float32)
    m = rng.uniform(-0.01, 0.01, n).astype(np.float32)
    v = rng.uniform(1e-5, 1e-3, n).astype(np.float32)
    tp, tm, tv = _t(p, cuda), _t(m, cuda), _t(v, cuda)
    for step in steps:
        g = sc.wide_grad(rng, n, 1).reshape(-1)
        hip_ops.dense_adam(tp, tm, tv, _t(g, cuda), ADAM_LR, betas[0], betas[1], EPS, step)
        oracle.dense_adam(p, m, v, g, ADAM_LR, betas[0], betas[1], EPS, step)
    return [x.cpu().numpy() for x in (tp, tm, tv)], [p, m, v]


def test_dense_adam_exact_betas_bitexact(cuda):
    got, ref = _dense_adam(cuda, 100003, sc.EXACT_BETAS, sc.EXACT_STEPS, np.random.default_rng(5))
    for g, r, name in zip(got, ref, ("p", "m", "v")):
        assert np.array_equal(g, r), name


def test_dense_adam_default_betas(cuda):
    got, ref = _dense_adam(cuda, 100003, sc.DEFAULT_BETAS, sc.EXACT_STEPS, np.random.default_rng(6))
    for g, r, name in zip(got, ref, ("p", "m", "v")):
        np.testing.assert_allclose(g, r, rtol=2e-6, atol=1e-7, err_msg=name)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])  # m, v: no powf in them


# --------------------------------------------------------------------------- grid-stride loops
GRID_CAP = 8192 * 256  # stride_grid: threads of the largest grid


def test_dense_optimizers_second_grid_trip(cuda):
    """n = 8192 * 256 + 257: the grid-stride loops of dense_adagrad and
    dense_adam take a second trip for the first 257 elements only."""
    rng = np.random.default_rng(8)
    n = GRID_CAP + 257
    p = rng.standard_normal(n).astype(np.float32)
    a = rng.uniform(0.05, 0.2, n).astype(np.float32)
    g = sc.wide_grad(rng, n, 1).reshape(-1)
    tp, ta = _t(p, cuda), _t(a, cuda)
    hip_ops.dense_adagrad(tp, ta, _t(g, cuda), LR, EPS)
    oracle.dense_adagrad(p, a, g, LR, EPS)
    assert np.array_equal(tp.cpu().numpy(), p) and np.array_equal(ta.cpu().numpy(), a)
    got, ref = _dense_adam(cuda, n, sc.EXACT_BETAS, (2,), rng)
    for x, r, name in zip(got, ref, ("p", "m", "v")):
        assert np.array_equal(x, r), name


def test_sparse_adam_table_passes_second_grid_trip(cuda):
    """A 20000 x 128 table (2.56 M elements): scale2_kernel and
    adam_var_kernel loop; 256 lookups touch a few rows, the rest only decay."""
    rng = np.random.default_rng(9)
    rows, dim, B = 20000, 128, 256
    assert rows * dim > GRID_CAP
    run_adam(cuda, [_tab(rows, dim, [_zipf(rng, B, rows)], [0])], B, sc.wide_grad(rng, B, dim), seed=9)


# --------------------------------------------------------------------------- dense_adagrad_many
MANY_SIZES = [0, 1, 255, 256, 257, 66048, 2_100_000, 3]


def _many_inputs(rng, sizes):
    return [[rng.standard_normal(n).astype(np.float32), rng.uniform(0.05, 0.2, n).astype(np.float32),
             sc.wide_grad(rng, n, 1).reshape(-1)] for n in sizes]


def test_dense_adagrad_many_job_search(cuda):
    """Eight jobs: an empty first job, job edges inside one wave (1, 255, 256,
    257), and a total above the grid cap (second trip across a job edge).  The
    result equals eight dense_adagrad calls and the oracle, bit for bit."""
    assert sum(MANY_SIZES) > GRID_CAP
    host = _many_inputs(np.random.default_rng(10), MANY_SIZES)
    many = [tuple(_t(x, cuda) for x in job) for job in host]
    single = [tuple(_t(x, cuda) for x in job) for job in host]
    hip_ops.dense_adagrad_many(many, LR, EPS)
    for p, a, g in single:
        hip_ops.dense_adagrad(p, a, g, LR, EPS)
    for i, (p, a, g) in enumerate(host):
        oracle.dense_adagrad(p, a, g, LR, EPS)
        for k, (want, name) in enumerate(((p, "param"), (a, "accum"))):
            assert np.array_equal(many[i][k].cpu().numpy(), want), f"job {i} {name} vs oracle"
            assert torch.equal(many[i][k], single[i][k]), f"job {i} {name} vs dense_adagrad"
        assert np.array_equal(many[i][2].cpu().numpy(), g)  # the gradient is only read


def test_dense_adagrad_many_one_job_and_empty_jobs(cuda):
    (host,) = _many_inputs(np.random.default_rng(12), [1000])
    one, ref = tuple(_t(x, cuda) for x in host), tuple(_t(x, cuda) for x in host)
    hip_ops.dense_adagrad_many([one], LR, EPS)
    hip_ops.dense_adagrad(*ref, LR, EPS)
    assert torch.equal(one[0], ref[0]) and torch.equal(one[1], ref[1])
    oracle.dense_adagrad(host[0], host[1], host[2], LR, EPS)
    assert np.array_equal(one[0].cpu().numpy(), host[0]) and np.array_equal(one[1].cpu().numpy(), host[1])
    empty = [tuple(torch.empty(0, device=cuda) for _ in range(3)) for _ in range(8)]
    hip_ops.dense_adagrad_many(empty, LR, EPS)
    torch.cuda.synchronize()
