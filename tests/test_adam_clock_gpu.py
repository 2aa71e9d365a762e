"""GPU: Adam's device step clock and the entries that read it.

tt_adam_clock_advance, tt_dense_adam_many_dev and tt_sparse_adam_dev against
the host-step entries (tt_dense_adam, tt_sparse_adam) on cloned state, bit for
bit: the device path must be the same arithmetic with the step's coefficient
read from the clock.  One run against the CPU restatement (exact betas) so a
mistake shared by both entries cannot hide, and one captured graph.

Sizes: n % 4 != 0 tails and tables of fewer than 4 elements (the 16-byte
units' scalar tail), 2.1 M dense elements and a 20000 x 128 table (more than
one trip of the grid-stride loops), 17 tables (a second whole-table launch),
tables at an address that is not 16-byte aligned (the scalar path).
"""
import numpy as np
import pytest
import torch

import sparse_cases as sc
from oracle import oracle
from pkg import _native
from pkg.modelling import hip_ops

pytestmark = pytest.mark.gpu

LR, EPS = 1e-3, 1e-7
EXACT = sc.EXACT_BETAS  # (0.5, 0.75): L = 61
DENSE_GRID = 8192 * 256   # stride_grid's cap in elements
TABLE_GRID = 2048 * 256 * 4  # the whole-table kernels' cap in elements


def _t(x, cuda):
    return torch.as_tensor(np.ascontiguousarray(x), device=cuda)


class Clock:
    """A device clock with its tables for (lr, betas)."""

    def __init__(self, cuda, betas, step=0, lr=LR):
        self.betas = betas
        self.L = hip_ops.adam_coef_len(*betas)
        assert self.L > 0
        self.alpha_host, self.lr_t_host = hip_ops.adam_coef_tables(lr, betas[0], betas[1], self.L)
        self.tabs = (self.alpha_host.to(cuda), self.lr_t_host.to(cuda))
        self.word = torch.zeros(2, dtype=torch.int64, device=cuda)
        self.set(step)

    def set(self, step):
        self.word.copy_(torch.tensor([step, 0], dtype=torch.int64))

    def advance(self):
        hip_ops.adam_clock_advance(self.word, *self.tabs)

    def read(self):
        w = self.word.cpu().numpy()
        pair = w[1:].view(np.float32)
        return int(w[0]), pair[0], pair[1]


# --------------------------------------------------------------------------- clock
@pytest.mark.parametrize("start", [0, 1, 59, 60, 61, 64, 2 ** 31 + 5])
def test_clock_advance(cuda, start):
    c = Clock(cuda, EXACT, start)
    assert c.L == 61
    c.advance()
    step, alpha, lr_t = c.read()
    k = min(start + 1, c.L) - 1
    assert step == start + 1
    assert alpha.tobytes() == c.alpha_host[k].numpy().tobytes()
    assert lr_t.tobytes() == c.lr_t_host[k].numpy().tobytes()
    if start + 1 >= c.L:
        assert alpha == np.float32(LR) and lr_t == np.float32(LR)
    elif start + 1 == c.L - 1:  # the last step before the end still differs
        assert alpha != np.float32(LR) and lr_t != np.float32(LR)


# --------------------------------------------------------------------------- dense
def _dense_state(rng, n):
    return [rng.standard_normal(n).astype(np.float32), rng.uniform(-0.01, 0.01, n).astype(np.float32),
            rng.uniform(1e-5, 1e-3, n).astype(np.float32), sc.wide_grad(rng, n, 1).reshape(-1)]


@pytest.mark.parametrize("sizes", [(1,), (255,), (4099,), (2100001,), (1, 255, 4099, 2100001, 255, 1, 4099, 0)],
                         ids=["n1", "n255", "n4099", "n2100001", "jobs8"])
@pytest.mark.parametrize("betas,step", [(sc.DEFAULT_BETAS, 3), (EXACT, 70)], ids=["default-s3", "exact-s70"])
def test_dense_adam_many_dev_equals_dense_adam(cuda, sizes, betas, step):
    assert 2100001 > DENSE_GRID  # the stride loop wraps for the largest job
    rng = np.random.default_rng(sum(sizes) + step)
    c = Clock(cuda, betas, step - 1)
    c.advance()
    jobs, refs, olds = [], [], []
    for n in sizes:
        state = [_t(x, cuda) for x in _dense_state(rng, n)]
        ref = [x.clone() for x in state]
        olds.append(state[0].clone())
        if n:
            hip_ops.dense_adam(ref[0], ref[1], ref[2], ref[3], LR, betas[0], betas[1], EPS, step)
        jobs.append(tuple(state))
        refs.append(ref)
    hip_ops.dense_adam_many_dev(jobs, betas[0], betas[1], EPS, c.word)
    assert c.read()[0] == step  # the entry does not touch the clock
    for i, (job, ref, old) in enumerate(zip(jobs, refs, olds)):
        for got, want, name in zip(job, ref, ("param", "m", "v", "grad")):
            assert torch.equal(got, want), (i, name)
        assert job[0].numel() == 0 or not torch.equal(job[0], old), i


def test_dense_adam_many_dev_rejects_bad_jobs(cuda):
    c = Clock(cuda, EXACT, 1)
    x = torch.zeros(4, device=cuda)
    with pytest.raises(_native.TTError) as e:
        hip_ops.dense_adam_many_dev([(x, x, x, x)] * 9, 0.5, 0.75, EPS, c.word)
    assert e.value.code == _native.TT_ERR_BAD_ARG
    jobs = (_native.DenseAdamJob * 1)()
    jobs[0].param, jobs[0].m, jobs[0].v, jobs[0].grad, jobs[0].n = x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 4
    rc = _native.lib().tt_dense_adam_many_dev(jobs, 1, 0.5, 0.75, EPS, c.word.data_ptr(), None)
    assert rc == _native.TT_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.equal(x, torch.zeros(4, device=cuda))


# --------------------------------------------------------------------------- sparse
def _ids(rng, batch, rows):
    """Heavy in duplicates (a few hot rows), with -1 and out-of-range ids."""
    hot = rng.integers(0, max(rows // 8, 1), batch)
    ids = np.where(rng.random(batch) < 0.7, hot, rng.integers(0, rows, batch)).astype(np.int32)
    bad = rng.random(batch) < 0.08
    ids[bad] = rng.choice(np.array([-1, rows, rows + 5], np.int32), int(bad.sum()))
    return ids


def _state(rng, rows, dim, cuda, misalign=False):
    """table, m, v with every element non-zero (rows no lookup touches still
    decay); misalign: each at a 4-byte offset into its allocation."""
    arrs = [rng.uniform(-0.05, 0.05, (rows, dim)), rng.uniform(-0.01, 0.01, (rows, dim)),
            rng.uniform(1e-5, 1e-3, (rows, dim))]
    out = []
    for a in arrs:
        if misalign:
            buf = torch.zeros(rows * dim + 1, dtype=torch.float32, device=cuda)
            t = buf[1:].view(rows, dim)
            t.copy_(_t(a.astype(np.float32), cuda))
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        else:
            t = _t(a.astype(np.float32), cuda)
        out.append(t)
    return out


def _specs(state, sources, grads=None):
    """sources[i]: list of (ids tensor, grad col offset); grads[i]: optional per-table grad."""
    return [dict(table=s[0], slot0=s[1], slot1=s[2], ids=[x for x, _ in src], grad_col_offset=[o for _, o in src],
                 **({"grad": grads[i]} if grads and grads[i] is not None else {}))
            for i, (s, src) in enumerate(zip(state, sources))]


def _both(cuda, state, sources, batch, grad, betas, step, grads=None, ws_tag="sparse"):
    """The device-clock entry on `state`, the host-step entry on a clone; equal bits."""
    ref = [[x.clone() for x in s] for s in state]
    before = [[x.clone() for x in s] for s in state]
    c = Clock(cuda, betas, step - 1)
    c.advance()
    hip_ops.sparse_adam_dev(_specs(state, sources, grads), batch, grad, betas[0], betas[1], EPS, c.word, ws_tag=ws_tag)
    hip_ops.sparse_status(cuda, ws_tag)
    ref_grad = grad if grad is not None else torch.zeros(batch, 1, device=cuda)  # unused: every table has its own
    hip_ops.sparse_adam(_specs(ref, sources, grads), batch, ref_grad, LR, betas[0], betas[1], EPS, step, ws_tag=ws_tag)
    hip_ops.sparse_status(cuda, ws_tag)
    assert c.read()[0] == step
    for i, (s, r, b) in enumerate(zip(state, ref, before)):
        for got, want, old, name in zip(s, r, b, ("table", "m", "v")):
            assert torch.equal(got, want), (i, name)
            assert not torch.equal(got, old), (i, name)  # every element decays / moves


GRID_SHAPES = [(rows, dim) for rows in (1, 37, 300, 20000) for dim in (1, 3, 4, 128)]


@pytest.mark.parametrize("step", [1, 2, 61, 66])
@pytest.mark.parametrize("batch", [1, 64, 257])
def test_sparse_adam_dev_equals_sparse_adam(cuda, batch, step):
    """All 16 (rows, dim) shapes as the 16 tables of one call: one decay launch
    and one update launch over 2.7 M elements (more than one grid pass), tails
    of 1..3 elements, tables smaller than one unit."""
    assert sum(r * d for r, d in GRID_SHAPES) > TABLE_GRID and 20000 * 128 > TABLE_GRID
    rng = np.random.default_rng(1000 * batch + step)
    state = [_state(rng, rows, dim, cuda) for rows, dim in GRID_SHAPES]
    sources, off = [], 0
    for rows, dim in GRID_SHAPES:
        sources.append([(_t(_ids(rng, batch, rows), cuda), off)])
        off += dim + 1
    grad = _t(sc.wide_grad(rng, batch, off), cuda)
    _both(cuda, state, sources, batch, grad, EXACT, step)


@pytest.mark.parametrize("step", [2, 17321, 17326])
def test_sparse_adam_dev_default_betas(cuda, step):
    """beta = (0.9, 0.999), L = 17321: a step inside the table, its last entry, and past it."""
    rng = np.random.default_rng(step)
    shapes, batch = [(300, 3), (37, 128), (5000, 4)], 257
    state = [_state(rng, r, d, cuda) for r, d in shapes]
    sources = [[(_t(_ids(rng, batch, r), cuda), 140 * i)] for i, (r, d) in enumerate(shapes)]
    _both(cuda, state, sources, batch, _t(sc.wide_grad(rng, batch, 420), cuda), sc.DEFAULT_BETAS, step)


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
def test_two_sources_and_per_table_grads(cuda, misalign):
    """Table 0 looked up twice (two sources of the call's gradient); tables 1
    and 2 read their own gradient buffers (another leading dimension, a
    column offset), as one call over both towers' tables does."""
    rng = np.random.default_rng(5 + misalign)
    batch = 257
    shapes = [(37, 3), (300, 4), (300, 128)]
    state = [_state(rng, r, d, cuda, misalign) for r, d in shapes]
    sources = [[(_t(_ids(rng, batch, 37), cuda), 0), (_t(_ids(rng, batch, 37), cuda), 5)],
               [(_t(_ids(rng, batch, 300), cuda), 2)],
               [(_t(_ids(rng, batch, 300), cuda), 0)]]
    grad = _t(sc.wide_grad(rng, batch, 8), cuda)
    grads = [None, _t(sc.wide_grad(rng, batch, 9), cuda), _t(sc.wide_grad(rng, batch, 128), cuda)]
    for step in (1, 66):
        _both(cuda, state, sources, batch, grad, EXACT, step, grads)


def test_every_table_brings_its_gradient(cuda):
    """grad=None for the call: the optimizer's joint call of both towers."""
    rng = np.random.default_rng(8)
    batch, shapes = 64, [(300, 4), (37, 3)]
    state = [_state(rng, r, d, cuda) for r, d in shapes]
    sources = [[(_t(_ids(rng, batch, r), cuda), 1)] for r, d in shapes]
    grads = [_t(sc.wide_grad(rng, batch, d + 1), cuda) for r, d in shapes]
    _both(cuda, state, sources, batch, None, EXACT, 2, grads)
    with pytest.raises(ValueError):
        hip_ops.sparse_adam_dev(_specs(state, sources), batch, None, 0.5, 0.75, EPS, Clock(cuda, EXACT, 1).word)


def test_bag_style_flat_problem(cuda):
    """A sequence feature's table: ids_flat [B * L] with -1 padding, G [B * L,
    dim] as the table's own gradient (grad_ld = dim, column 0), on the bag
    workspace."""
    rng = np.random.default_rng(9)
    B, L, rows, dim = 64, 5, 50, 8
    ids = rng.integers(0, rows, (B, L)).astype(np.int32)
    ids[np.arange(L)[None, :] >= rng.integers(0, L + 1, B)[:, None]] = -1
    state = [_state(rng, rows, dim, cuda)]
    G = _t(sc.wide_grad(rng, B * L, dim), cuda)
    _both(cuda, state, [[(_t(ids.reshape(-1), cuda), 0)]], B * L, None, EXACT, 3, [G], ws_tag="sparse_bag")


def test_seventeen_tables_take_two_whole_table_launches(cuda):
    rng = np.random.default_rng(10)
    batch = 64
    shapes = [(5 + i, 1 + i % 5) for i in range(17)]
    state = [_state(rng, r, d, cuda) for r, d in shapes]
    sources = [[(_t(_ids(rng, batch, r), cuda), 6 * i)] for i, (r, d) in enumerate(shapes)]
    _both(cuda, state, sources, batch, _t(sc.wide_grad(rng, batch, 6 * 17), cuda), EXACT, 2)


def test_batch_zero_still_decays_and_updates(cuda):
    rng = np.random.default_rng(11)
    shapes = [(37, 3), (300, 4)]
    state = [_state(rng, r, d, cuda) for r, d in shapes]
    empty = torch.empty(0, dtype=torch.int32, device=cuda)
    grad = torch.empty(0, 8, dtype=torch.float32, device=cuda)
    _both(cuda, state, [[(empty, 0)], [(empty, 3)]], 0, grad, EXACT, 2)


# --------------------------------------------------------------------------- oracle
def test_three_steps_against_the_cpu_restatement(cuda):
    """Exact betas, steps 1..3 from a clock at 0: tables, slots and a dense
    buffer equal oracle.sparse_adam / oracle.dense_adam bit for bit."""
    rng = np.random.default_rng(12)
    batch, shapes, n = 257, [(300, 3), (37, 4)], 4099
    c = Clock(cuda, EXACT, 0)
    ref = [[x.astype(np.float32) for x in (rng.uniform(-0.05, 0.05, s), rng.uniform(-0.01, 0.01, s),
                                            rng.uniform(1e-5, 1e-3, s))] for s in shapes]
    state = [[_t(x, cuda) for x in r] for r in ref]
    dref = _dense_state(rng, n)[:3]
    dstate = [_t(x, cuda) for x in dref]
    for step in sc.EXACT_STEPS:
        ids = [_ids(rng, batch, r) for r, d in shapes]
        grad = sc.wide_grad(rng, batch, 8)
        dg = sc.wide_grad(rng, n, 1).reshape(-1)
        c.advance()
        hip_ops.dense_adam_many_dev([(dstate[0], dstate[1], dstate[2], _t(dg, cuda))], EXACT[0], EXACT[1], EPS, c.word)
        sources = [[(_t(ids[0], cuda), 0)], [(_t(ids[1], cuda), 4)]]
        hip_ops.sparse_adam_dev(_specs(state, sources), batch, _t(grad, cuda), EXACT[0], EXACT[1], EPS, c.word)
        oracle.dense_adam(dref[0], dref[1], dref[2], dg, LR, EXACT[0], EXACT[1], EPS, step)
        for i, (off, (r, d)) in enumerate(zip((0, 4), shapes)):
            oracle.sparse_adam(ref[i][0], ref[i][1], ref[i][2], ids[i], np.ascontiguousarray(grad[:, off:off + d]), LR,
                               EXACT[0], EXACT[1], EPS, step)
        for i in range(len(shapes)):
            for got, want, name in zip(state[i], ref[i], ("table", "m", "v")):
                assert np.array_equal(got.cpu().numpy(), want), (step, i, name)
        for got, want, name in zip(dstate, dref, ("param", "m", "v")):
            assert np.array_equal(got.cpu().numpy(), want), (step, name)
    assert c.read()[0] == 3


# --------------------------------------------------------------------------- capture
def test_captured_step_replays_as_successive_steps(cuda):
    """[advance, dense-many, sparse] captured once and replayed 5 times equals
    5 eager host-step calls at steps 1..5."""
    rng = np.random.default_rng(13)
    batch, shapes, n, betas = 64, [(300, 4), (37, 3)], 4099, sc.DEFAULT_BETAS
    state = [_state(rng, r, d, cuda) for r, d in shapes]
    sources = [[(_t(_ids(rng, batch, r), cuda), 4 * i)] for i, (r, d) in enumerate(shapes)]
    grad = _t(sc.wide_grad(rng, batch, 8), cuda)
    dstate = [_t(x, cuda) for x in _dense_state(rng, n)]
    ref = [[x.clone() for x in s] for s in state]
    dref = [x.clone() for x in dstate]

    def step_on(c, st, ds):
        c.advance()
        hip_ops.dense_adam_many_dev([tuple(ds)], betas[0], betas[1], EPS, c.word)
        hip_ops.sparse_adam_dev(_specs(st, sources), batch, grad, betas[0], betas[1], EPS, c.word)

    # warm the workspace and the kernels on scratch state before capturing
    step_on(Clock(cuda, betas, 0), [[x.clone() for x in s] for s in state], [x.clone() for x in dstate])
    torch.cuda.synchronize()
    c = Clock(cuda, betas, 0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        step_on(c, state, dstate)
    assert c.read()[0] == 0  # capturing runs nothing
    for _ in range(5):
        g.replay()
    for step in range(1, 6):
        hip_ops.dense_adam(dref[0], dref[1], dref[2], dref[3], LR, betas[0], betas[1], EPS, step)
        hip_ops.sparse_adam(_specs(ref, sources), batch, grad, LR, betas[0], betas[1], EPS, step)
    torch.cuda.synchronize()
    assert c.read()[0] == 5
    for i in range(len(shapes)):
        for got, want, name in zip(state[i], ref[i], ("table", "m", "v")):
            assert torch.equal(got, want), (i, name)
    for got, want, name in zip(dstate, dref, ("param", "m", "v")):
        assert torch.equal(got, want), name
    hip_ops.sparse_status(cuda)
