"""GPU: tt_gather_bag / tt_bag_grad_expand (hip_ops.gather_bag,
bag_grad_expand) against the numpy restatement in bag_ref, bit for bit, the
table update through the existing sparse entries on the flat problem, and the
gradient against torch fp64 autograd."""
import numpy as np
import pytest
import torch

import bag_ref
from pkg.modelling import hip_ops

pytestmark = pytest.mark.gpu

DIMS = (1, 5, 64, 128, 1024)
LS = (1, 3, 9, 33)
BS = (1, 63, 65, 257)
V = 50
SENTINEL = 777.0


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _table(rng, dim, rows=V):
    t = rng.standard_normal((rows, dim)).astype(np.float32)
    t[1] = -0.0          # a bag of this row alone keeps its sign bits
    t[2, ::2] = 0.0
    return t


def _misaligned(a: np.ndarray, cuda) -> torch.Tensor:
    """The array at a base address 4 bytes past a 16-byte boundary."""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=cuda)
    v = buf[1:].view(a.shape)
    v.copy_(torch.as_tensor(a))
    assert v.data_ptr() % 16 == 4
    return v


def _ids_layouts(ids: np.ndarray, cuda):
    """[B, L] row-major, and the transposed view of an [L, B] block."""
    row_major = torch.as_tensor(ids, device=cuda)
    block = torch.as_tensor(np.ascontiguousarray(ids.T), device=cuda)
    return row_major, block.t()


def _forward(table_t, ids_t, pooling, B, dim, off, cuda):
    ld = (off + dim + 5 + 3) // 4 * 4
    out = torch.full((B, ld), SENTINEL, dtype=torch.float32, device=cuda)
    scale = torch.full((B,), SENTINEL, dtype=torch.float32, device=cuda)
    hip_ops.gather_bag([(table_t, ids_t, pooling, out, off, scale)], B)
    return out, scale


@pytest.mark.parametrize("pooling", bag_ref.POOLINGS)
@pytest.mark.parametrize("dim", DIMS)
def test_forward_bits(cuda, dim, pooling):
    rng = np.random.default_rng(1000 + dim)
    table = _table(rng, dim)
    aligned = torch.as_tensor(table, device=cuda)
    shifted = _misaligned(table, cuda)
    for L in LS:
        for B in BS:
            ids = bag_ref.random_bags(rng, B, L, V)
            ref_out, ref_scale = bag_ref.gather_bag(table, ids, pooling)
            ref_out_t, ref_scale_t = torch.as_tensor(ref_out, device=cuda), torch.as_tensor(ref_scale, device=cuda)
            assert not np.signbit(ref_out[0]).any() and ref_scale[0] == 0.0  # the empty bag: +0.0
            for off, table_t in ((0, aligned), (3, shifted)):
                for ids_t in _ids_layouts(ids, cuda):
                    out, scale = _forward(table_t, ids_t, pooling, B, dim, off, cuda)
                    where = f"dim={dim} L={L} B={B} off={off} ids strides={ids_t.stride()}"
                    assert _same_bits(out[:, off:off + dim], ref_out_t), where
                    assert _same_bits(scale, ref_scale_t), where
                    assert bool((out[:, :off] == SENTINEL).all()) and bool((out[:, off + dim:] == SENTINEL).all()), where


def test_first_bags_do_not_depend_on_batch(cuda):
    rng = np.random.default_rng(7)
    for dim in (5, 64, 128):
        table = torch.as_tensor(_table(rng, dim), device=cuda)
        ids = torch.as_tensor(bag_ref.random_bags(rng, 257, 9, V), device=cuda)
        big, big_scale = _forward(table, ids, "mean", 257, dim, 0, cuda)
        small, small_scale = _forward(table, ids[:63].contiguous(), "mean", 63, dim, 0, cuda)
        assert _same_bits(big[:63], small) and _same_bits(big_scale[:63], small_scale)


def test_two_jobs_equal_two_launches(cuda):
    rng = np.random.default_rng(8)
    B = 65
    t64 = torch.as_tensor(_table(rng, 64), device=cuda)
    t5 = torch.as_tensor(_table(rng, 5, rows=31), device=cuda)
    i64 = torch.as_tensor(bag_ref.random_bags(rng, B, 9, V), device=cuda)
    i5 = torch.as_tensor(bag_ref.random_bags(rng, B, 3, 31), device=cuda)
    outs, scales = [], []
    for together in (True, False):
        out = torch.full((B, 76), SENTINEL, dtype=torch.float32, device=cuda)
        s64 = torch.empty(B, dtype=torch.float32, device=cuda)
        s5 = torch.empty(B, dtype=torch.float32, device=cuda)
        jobs = [(t64, i64, "sqrtn", out, 4, s64), (t5, i5, "mean", out, 69, s5)]
        if together:
            hip_ops.gather_bag(jobs, B)
        else:
            hip_ops.gather_bag(jobs[:1], B)
            hip_ops.gather_bag(jobs[1:], B)
        outs.append(out)
        scales.append(torch.cat([s64, s5]))
    assert _same_bits(outs[0], outs[1]) and _same_bits(scales[0], scales[1])
    assert bool((outs[0][:, :4] == SENTINEL).all()) and bool((outs[0][:, 68] == SENTINEL).all())
    ref, _ = bag_ref.gather_bag(t5.cpu().numpy(), i5.cpu().numpy(), "mean")
    assert _same_bits(outs[0][:, 69:74], torch.as_tensor(ref, device=cuda))


def _expand_case(rng, B, L, dim, pooling, off, cuda, transposed=False):
    ids = bag_ref.random_bags(rng, B, L, V)
    dout = rng.standard_normal((B, off + dim + 2)).astype(np.float32)
    cnt = bag_ref.valid_slots(ids, V).sum(1)
    scale = bag_ref.bag_scale(cnt, pooling)
    ids_t = _ids_layouts(ids, cuda)[1 if transposed else 0]
    ids_flat = torch.full((B * L,), -9, dtype=torch.int32, device=cuda)
    G = torch.full((B * L, dim), SENTINEL, dtype=torch.float32, device=cuda)
    hip_ops.bag_grad_expand([(V, ids_t, pooling, torch.as_tensor(dout, device=cuda), off,
                              torch.as_tensor(scale, device=cuda), ids_flat, G)], B)
    ref = bag_ref.expand(ids, V, dout[:, off:off + dim], scale, pooling)
    return ids_flat, G, ref


@pytest.mark.parametrize("pooling", bag_ref.POOLINGS)
@pytest.mark.parametrize("dim", DIMS)
def test_expand_bits(cuda, dim, pooling):
    rng = np.random.default_rng(2000 + dim)
    for L in LS:
        for B in (1, 65, 257):
            for off, transposed in ((0, False), (3, True)):
                ids_flat, G, (ref_ids, ref_G, valid) = _expand_case(rng, B, L, dim, pooling, off, cuda, transposed)
                where = f"dim={dim} L={L} B={B} off={off}"
                assert torch.equal(ids_flat, torch.as_tensor(ref_ids, device=cuda)), where
                v = torch.as_tensor(valid, device=cuda)
                assert _same_bits(G[v], torch.as_tensor(ref_G[valid], device=cuda)), where
                assert bool((G[~v] == SENTINEL).all()), where  # rows of invalid slots are not written


@pytest.mark.parametrize("pooling", ("mean", "sum"))
def test_flat_adagrad_update_bits(cuda, pooling):
    rng = np.random.default_rng(31)
    B, L, dim, rows = 257, 9, 64, 300
    table = _table(rng, dim, rows)
    accum = np.full_like(table, 0.1)
    ids = bag_ref.random_bags(rng, B, L, rows)
    ids[ids == 5] = 6  # row 5 is named by no slot
    dout = rng.standard_normal((B, dim + 4)).astype(np.float32)
    tt, ta = torch.as_tensor(table, device=cuda), torch.as_tensor(accum, device=cuda)
    out = torch.empty(B, dim + 4, dtype=torch.float32, device=cuda)
    scale = torch.empty(B, dtype=torch.float32, device=cuda)
    ids_t = torch.as_tensor(ids, device=cuda)
    hip_ops.gather_bag([(tt, ids_t, pooling, out, 4, scale)], B)
    ids_flat = torch.empty(B * L, dtype=torch.int32, device=cuda)
    G = torch.zeros(B * L, dim, dtype=torch.float32, device=cuda)
    hip_ops.bag_grad_expand([(rows, ids_t, pooling, torch.as_tensor(dout, device=cuda), 4, scale, ids_flat, G)], B)
    hip_ops.sparse_adagrad([dict(table=tt, slot0=ta, ids=[ids_flat], grad_col_offset=[0], grad=G)], B * L, None,
                           0.05, 1e-7, ws_tag="sparse_bag")
    hip_ops.sparse_status(cuda, "sparse_bag")
    ref_t, ref_a = table.copy(), accum.copy()
    bag_ref.flat_adagrad(ref_t, ref_a, ids_flat.cpu().numpy(), G.cpu().numpy(), 0.05, 1e-7)
    assert np.array_equal(tt.cpu().numpy().view(np.int32), ref_t.view(np.int32))
    assert np.array_equal(ta.cpu().numpy().view(np.int32), ref_a.view(np.int32))
    # the restatement's own flat problem gives the same update; untouched rows keep their bits
    r_ids, r_G, _ = bag_ref.expand(ids, rows, dout[:, 4:], scale.cpu().numpy(), pooling)
    ref2_t, ref2_a = table.copy(), accum.copy()
    bag_ref.flat_adagrad(ref2_t, ref2_a, r_ids, r_G, 0.05, 1e-7)
    assert np.array_equal(ref2_t.view(np.int32), ref_t.view(np.int32))
    untouched = np.setdiff1d(np.arange(rows), r_ids[r_ids >= 0])
    assert 5 in untouched
    assert np.array_equal(tt.cpu().numpy()[untouched].view(np.int32), table[untouched].view(np.int32))
    assert np.array_equal(ta.cpu().numpy()[untouched].view(np.int32), accum[untouched].view(np.int32))


def test_flat_adam_update(cuda):
    rng = np.random.default_rng(32)
    B, L, dim, rows = 65, 9, 64, 300
    table = _table(rng, dim, rows)
    m, v = np.zeros_like(table), np.zeros_like(table)
    tt, tm, tv = (torch.as_tensor(x, device=cuda) for x in (table, m, v))
    for step in (1, 2):
        ids = bag_ref.random_bags(rng, B, L, rows)
        dout = rng.standard_normal((B, dim)).astype(np.float32)
        scale = torch.as_tensor(bag_ref.bag_scale(bag_ref.valid_slots(ids, rows).sum(1), "sqrtn"), device=cuda)
        ids_flat = torch.empty(B * L, dtype=torch.int32, device=cuda)
        G = torch.zeros(B * L, dim, dtype=torch.float32, device=cuda)
        hip_ops.bag_grad_expand([(rows, torch.as_tensor(ids, device=cuda), "sqrtn", torch.as_tensor(dout, device=cuda),
                                  0, scale, ids_flat, G)], B)
        hip_ops.sparse_adam([dict(table=tt, slot0=tm, slot1=tv, ids=[ids_flat], grad_col_offset=[0])], B * L, G,
                            1e-3, 0.9, 0.999, 1e-7, step, ws_tag="sparse_bag")
        bag_ref.flat_adam(table, m, v, ids_flat.cpu().numpy(), G.cpu().numpy(), 1e-3, 0.9, 0.999, 1e-7, step)
    np.testing.assert_allclose(tt.cpu().numpy(), table, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(tm.cpu().numpy(), m, rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("pooling", bag_ref.POOLINGS)
def test_gradient_against_fp64_autograd(cuda, pooling):
    """Independent of the restatement: the per-row sums of G against torch fp64
    autograd of the pooled forward with respect to the table.  Bound per
    element: 2 n 2^-24 sum|g|, n the row's lookup count, sum|g| the sum of
    the absolute fp64 contributions to that element."""
    rng = np.random.default_rng(33)
    B, L, dim = 257, 9, 64
    table = _table(rng, dim)
    ids = bag_ref.random_bags(rng, B, L, V)
    dout = rng.standard_normal((B, dim)).astype(np.float32)
    ok = torch.as_tensor(bag_ref.valid_slots(ids, V))
    safe = torch.as_tensor(np.where(ok.numpy(), ids, 0).astype(np.int64))
    cnt = ok.sum(1).double()

    def scale_of(c):
        if pooling == "sum":
            return torch.where(c > 0, torch.ones_like(c), torch.zeros_like(c))
        p = 1.0 if pooling == "mean" else 0.5
        return torch.where(c > 0, c.clamp_min(1.0) ** -p, torch.zeros_like(c))

    w = torch.as_tensor(table).double().requires_grad_(True)
    pooled = (w[safe] * ok[..., None]).sum(1) * scale_of(cnt)[:, None]
    d64 = torch.as_tensor(dout).double()
    (pooled * d64).sum().backward()
    contrib = (d64 * scale_of(cnt)[:, None]).abs()[:, None, :].expand(B, L, dim) * ok[..., None]
    sum_abs = torch.zeros(V, dim, dtype=torch.float64).index_add_(0, safe.reshape(-1), contrib.reshape(-1, dim))
    n = torch.zeros(V, dtype=torch.float64).index_add_(0, safe.reshape(-1), ok.reshape(-1).double())

    tt = torch.as_tensor(table, device=cuda)
    ids_t = torch.as_tensor(ids, device=cuda)
    out = torch.empty(B, dim, dtype=torch.float32, device=cuda)
    scale = torch.empty(B, dtype=torch.float32, device=cuda)
    hip_ops.gather_bag([(tt, ids_t, pooling, out, 0, scale)], B)
    ids_flat = torch.empty(B * L, dtype=torch.int32, device=cuda)
    G = torch.zeros(B * L, dim, dtype=torch.float32, device=cuda)
    hip_ops.bag_grad_expand([(V, ids_t, pooling, torch.as_tensor(dout, device=cuda), 0, scale, ids_flat, G)], B)
    flat, Gc = ids_flat.cpu().long(), G.cpu().double()
    keep = flat >= 0
    got = torch.zeros(V, dim, dtype=torch.float64).index_add_(0, flat[keep], Gc[keep])
    bound = 2.0 * n[:, None] * 2.0 ** -24 * sum_abs
    err = (got - w.grad).abs()
    print(f"bag gradient {pooling}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
