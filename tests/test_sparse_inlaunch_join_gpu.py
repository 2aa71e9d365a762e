"""The join of long segments inside the block-sum launch (csrc/tt_sparse.hip).

A segment of equal row ids longer than a 32-lookup block is summed in pieces
by several blocks, which may run in different workgroups on different XCDs.
Each block publishes its piece and draws a ticket on the segment's counter;
the block that draws the last ticket adds the pieces in block order and
applies the update.  These tests place the hand-off where it can go wrong and
compare every output bit for bit with oracle/ (np.array_equal), as
tests/test_sparse_edges_gpu.py does for the rest of the update:

  segments   33 and 64 repeats (two blocks), 32 x 40 (more than one batch of
             32 pieces per join), 32 x 70 at dim 128 (one wave per block, the
             blocks spread over workgroups), a segment that is its whole
             region, two long segments meeting inside one block, an invalid-id
             run across blocks;
  tables     dims 128, 2 and 4 with 5000, 100 and 256 rows in one call (the
             small table's waves are ordered first in the launch);
  reuse      one workspace through three calls with the same ids and new
             gradients (a joiner reading a stale piece would differ), the same
             with the sort on another stream, three applies on one sort (the
             joiner resets its counter), a captured sort + apply replayed on
             new gradients, and eager against replay.
"""
import numpy as np
import pytest
import torch

import sparse_cases as sc
import test_sparse_edges_gpu as edges
from oracle import oracle
from pkg.modelling import hip_ops

pytestmark = pytest.mark.gpu

LR, EPS = edges.LR, edges.EPS
_t, _tab = edges._t, edges._tab

# (row, count) runs of a sc.GEOM_ROWS-row table, invalid ids
SEGMENTS = {
    "rep33": ([(5, 33)], 0),                 # two blocks, the second mostly padding
    "rep64": ([(5, 64)], 0),                 # exactly two full blocks: the segment is the whole region
    "rep1280": ([(5, 32 * 40)], 0),          # 40 pieces: two batches of the join
    "rep2240": ([(5, 32 * 70)], 0),          # 70 blocks
    "whole_region_ragged": ([(7, 32 * 3 + 5)], 0),   # the whole region, ending inside its last block
    # row 3 ends at slot 9 of block 3 (head piece), row 9 starts at slot 10 of
    # the same block and runs to the end of block 6 (tail piece)
    "two_meet": ([(3, 32 * 3 + 10), (9, 32 * 3 + 22)], 0),
    # a joined run, then 70 invalid ids: the invalid run spans three blocks
    "invalid_span": ([(1, 3), (2, 40)], 70),
}


@pytest.mark.parametrize("op", ["adagrad", "adam", "scatter_sum", "dedup_sum"])
@pytest.mark.parametrize("dim", [2, 128])
@pytest.mark.parametrize("name", sorted(SEGMENTS))
def test_segments_across_blocks(cuda, name, dim, op):
    """Constructed segments at dim 2 (32 blocks per wave: the tickets of one
    wave's slots diverge) and dim 128 (one block per wave, two column passes)."""
    runs, n_invalid = SEGMENTS[name]
    seed = sorted(SEGMENTS).index(name)
    counts = sc.counts_of(sc.GEOM_ROWS, runs)
    ids = sc.ids_from_counts(counts, n_invalid, np.random.default_rng(seed), sc.GEOM_ROWS)
    grad = sc.wide_grad(np.random.default_rng(100 + seed), len(ids), dim)
    edges.OPS[op](cuda, [_tab(sc.GEOM_ROWS, dim, [ids], [0])], len(ids), grad, seed=seed)


# ------------------------------------------------------------------ table mix
MIX_B = 2048
MIX_SHAPES = [(5000, 128), (100, 2), (256, 4)]   # (rows, dim): the small table is not first in the call


def _mix_tables(rng):
    tabs, off = [], 0
    for rows, dim in MIX_SHAPES:
        tabs.append(_tab(rows, dim, [edges._zipf(rng, MIX_B, rows)], [off]))
        off += dim
    return tabs, off


@pytest.mark.parametrize("op", ["adagrad", "adam", "scatter_sum"])
def test_table_mix(cuda, op):
    """Three tables in one call: Zipf ids give each long segments; the
    100-row table's blocks are nearly all pieces."""
    rng = np.random.default_rng(31)
    tabs, width = _mix_tables(rng)
    edges.OPS[op](cuda, tabs, MIX_B, sc.wide_grad(rng, MIX_B, width), seed=31)


@pytest.mark.parametrize("which", range(len(MIX_SHAPES)))
def test_table_mix_dedup_sum(cuda, which):
    rng = np.random.default_rng(32)
    tabs, width = _mix_tables(rng)
    edges.run_dedup(cuda, [tabs[which]], MIX_B, sc.wide_grad(rng, MIX_B, width))


# ------------------------------------------------------------------ one workspace, many calls
class _Mix:
    """The mixed call's tables on the GPU and in the oracle, advanced together."""

    def __init__(self, cuda, seed):
        rng = np.random.default_rng(seed)
        self.cuda = cuda
        self.tabs, self.width = _mix_tables(rng)
        self.w = [rng.uniform(-0.05, 0.05, s).astype(np.float32) for s in MIX_SHAPES]
        self.acc = [rng.uniform(0.05, 0.2, s).astype(np.float32) for s in MIX_SHAPES]
        self.state = [(_t(a, cuda), _t(b, cuda)) for a, b in zip(self.w, self.acc)]
        self.specs = edges._specs(cuda, self.tabs, MIX_B, self.state, ["slot0"])
        self.grads = [sc.wide_grad(rng, MIX_B, self.width) for _ in range(3)]

    def reference_step(self, grad):
        for i, tab in enumerate(self.tabs):
            ids, g = edges._lookups(tab, grad)
            oracle.sparse_adagrad(self.w[i], self.acc[i], ids, g, LR, EPS)

    def check(self, what):
        hip_ops.sparse_status(self.cuda)
        for i in range(len(self.tabs)):
            assert np.array_equal(self.state[i][0].cpu().numpy(), self.w[i]), f"{what}: table {i}"
            assert np.array_equal(self.state[i][1].cpu().numpy(), self.acc[i]), f"{what}: accumulator {i}"


def _ws_ptr(cuda):
    return hip_ops.Workspace.existing(cuda, "sparse", None).data_ptr()


def test_same_workspace_three_calls(cuda):
    """Same ids, new gradients, one workspace: every piece slot and counter of
    call k + 1 is the one call k used."""
    m = _Mix(cuda, 41)
    ptrs = set()
    for k, grad in enumerate(m.grads):
        hip_ops.sparse_adagrad(m.specs, MIX_B, _t(grad, cuda), LR, EPS)
        ptrs.add(_ws_ptr(cuda))
        m.reference_step(grad)
        m.check(f"call {k}")
    assert len(ptrs) == 1


def test_split_stages_on_two_streams(cuda):
    """tt_sparse_sort on one stream, tt_sparse_adagrad_sorted on another, three times."""
    m = _Mix(cuda, 42)
    sort_s, apply_s = torch.cuda.Stream(), torch.cuda.Stream()
    sort_s.wait_stream(torch.cuda.current_stream())
    for k, grad in enumerate(m.grads):
        g = _t(grad, cuda)
        with torch.cuda.stream(sort_s):
            hip_ops.sparse_sort(m.specs, MIX_B)
        apply_s.wait_stream(sort_s)
        apply_s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(apply_s):
            hip_ops.sparse_adagrad(m.specs, MIX_B, g, LR, EPS, presorted=True)
        sort_s.wait_stream(apply_s)
        torch.cuda.current_stream().wait_stream(apply_s)
        m.reference_step(grad)
        m.check(f"call {k}")


def test_three_applies_on_one_sort(cuda):
    """The joiner leaves its counter at zero: a second and third apply on the
    same sorted keys join every long segment again."""
    m = _Mix(cuda, 43)
    hip_ops.sparse_sort(m.specs, MIX_B)
    for k, grad in enumerate(m.grads):
        hip_ops.sparse_adagrad(m.specs, MIX_B, _t(grad, cuda), LR, EPS, presorted=True)
        m.reference_step(grad)
        m.check(f"apply {k}")


def test_captured_sort_and_apply_replayed(cuda):
    """A hipGraph of sort + apply replayed three times, a new gradient copied in before each."""
    m = _Mix(cuda, 44)
    static = torch.zeros(MIX_B, m.width, device=cuda)
    hip_ops.sparse_sort(m.specs, MIX_B)  # warm: the workspace exists before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with hip_ops.capture_guard(), torch.cuda.graph(g):
        hip_ops.sparse_sort(m.specs, MIX_B)
        hip_ops.sparse_adagrad(m.specs, MIX_B, static, LR, EPS, presorted=True)
    for k, grad in enumerate(m.grads):
        static.copy_(_t(grad, cuda))
        g.replay()
        m.reference_step(grad)
        m.check(f"replay {k}")


def test_eager_equals_replay(cuda):
    """The mixed call run twice eagerly and twice as a replay, from equal
    states: equal tables and accumulators."""
    eager, replay = _Mix(cuda, 45), _Mix(cuda, 45)
    static = torch.zeros(MIX_B, eager.width, device=cuda)
    for grad in eager.grads[:2]:
        hip_ops.sparse_adagrad(eager.specs, MIX_B, _t(grad, cuda), LR, EPS)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with hip_ops.capture_guard(), torch.cuda.graph(g):
        hip_ops.sparse_adagrad(replay.specs, MIX_B, static, LR, EPS)
    for grad in replay.grads[:2]:
        static.copy_(_t(grad, cuda))
        g.replay()
    torch.cuda.synchronize()
    hip_ops.sparse_status(cuda)
    for i in range(len(MIX_SHAPES)):
        assert torch.equal(eager.state[i][0], replay.state[i][0]), f"table {i}"
        assert torch.equal(eager.state[i][1], replay.state[i][1]), f"accumulator {i}"
    for grad in eager.grads[:2]:
        eager.reference_step(grad)
    eager.check("eager")
