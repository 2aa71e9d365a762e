"""GPU: tt_l2norm_rows / tt_l2norm_rows_grad (hip_ops.l2norm_rows,
l2norm_rows_grad) against torch fp64, and their exact properties.

Bounds (per element; the issue's): forward |y - y64| <= 2e-6 * scale;
gradient |dx - dx64| <= 2e-6 * scale * inv_i * ||dy_i||_2.  Basis: a numpy
fp32 restatement with a sequential sum (the worst order) stays within
4.4 * 2^-24 ~ 2.7e-7 of fp64 over these dims and input kinds; the bound
leaves about 8x for another summation order and the division / square root.
Each test prints the largest error it saw as a fraction of its bound's unit
(run with -s to see them; DESIGN §6 records them)."""
import numpy as np
import pytest
import torch

from pkg.modelling import hip_ops

pytestmark = pytest.mark.gpu

ROWS = (1, 63, 64, 65, 257)
DIMS = (1, 4, 7, 64, 128, 129, 384)
SCALES = (1.0, 20.0)
KINDS = (1.0, 1e3, 1e-3)
SENTINEL = 777.0
TOL = 2e-6


def _lds(dim):
    return (dim, dim + 3, 4 * ((dim + 3) // 4) + 4)


def _buf(rows, dim, ld, cuda, fill=None):
    """A [rows, dim] view of a [rows, ld] buffer whose every float is the sentinel."""
    b = torch.full((rows, ld), SENTINEL, dtype=torch.float32, device=cuda)
    v = b[:, :dim]
    if fill is not None:
        v.copy_(fill)
    return b, v


def _inputs(rows, dim, kind, cuda, seed, parallel=False):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.relu(torch.randn(rows, dim, generator=g)) * kind
    x[0] = 0
    x[-1] = 0
    dy = 3.0 * x if parallel else torch.randn(rows, dim, generator=g)
    return x.to(cuda), dy.to(cuda)


def _ref(x, dy, scale):
    x64, dy64 = x.double(), dy.double()
    ss = (x64 * x64).sum(1)
    inv = torch.where(ss > 0, ss.clamp_min(1e-300).rsqrt(), torch.zeros_like(ss))
    y = x64 * (scale * inv)[:, None]
    u = x64 * inv[:, None]
    dx = (scale * inv)[:, None] * (dy64 - u * (u * dy64).sum(1, keepdim=True))
    return y, inv, dx


def _check_case(rows, dim, ld, scale, kind, cuda, seed, parallel=False):
    """One forward + gradient on strided buffers; asserts the bounds and the
    exact properties of zero rows and sentinel columns; returns the largest
    errors in units of their bounds' scale (fwd, inv, grad)."""
    x, dy = _inputs(rows, dim, kind, cuda, seed, parallel)
    xb, xv = _buf(rows, dim, ld, cuda, x)
    yb, yv = _buf(rows, dim, ld, cuda)
    db, dv = _buf(rows, dim, ld, cuda, dy)
    gb, gv = _buf(rows, dim, ld, cuda)
    inv = torch.full((rows,), SENTINEL, dtype=torch.float32, device=cuda)
    hip_ops.l2norm_rows([(xv, scale, yv, inv)])
    hip_ops.l2norm_rows_grad([(xv, inv, dv, scale, gv)])
    y64, inv64, dx64 = _ref(x, dy, scale)
    tag = (rows, dim, ld, scale, kind, parallel)
    # sentinel columns dim..ld of the outputs untouched; the inputs unchanged
    for b in (yb, gb):
        assert torch.all(b[:, dim:] == SENTINEL), tag
    assert torch.equal(xv, x) and torch.equal(dv, dy), tag
    # zero rows: +0.0f in every element, inv = +0.0f
    for r in {0, rows - 1}:
        assert torch.all(yv[r].contiguous().view(torch.int32) == 0), tag
        assert torch.all(gv[r].contiguous().view(torch.int32) == 0), tag
        assert inv[r:r + 1].view(torch.int32).item() == 0, tag
    e_fwd = ((yv.double() - y64).abs().max() / scale).item()
    assert e_fwd <= TOL, (tag, e_fwd)
    live = inv64 > 0
    e_inv = 0.0
    if live.any():
        e_inv = ((inv.double() - inv64).abs()[live] / inv64[live]).max().item()
        assert e_inv <= TOL, (tag, e_inv)
    unit = scale * inv64 * dy.double().norm(dim=1)  # per row
    err = (gv.double() - dx64).abs().max(dim=1).values
    assert torch.all(err <= TOL * unit), (tag, (err - TOL * unit).max().item())
    e_grad = (err[live] / unit[live]).max().item() if live.any() else 0.0
    return e_fwd, e_inv, e_grad


@pytest.mark.parametrize("dim", DIMS)
def test_against_fp64(cuda, dim):
    worst = np.zeros(3)
    seed = 1000 * dim
    for rows in ROWS:
        for ld in _lds(dim):
            for scale in SCALES:
                for kind in KINDS:
                    seed += 1
                    worst = np.maximum(worst, _check_case(rows, dim, ld, scale, kind, cuda, seed))
    print(f"\nl2norm dim={dim}: fwd {worst[0]:.3e}  inv {worst[1]:.3e}  grad {worst[2]:.3e}  (bound {TOL:.0e})")


def test_against_fp64_dim_4096(cuda):
    worst = np.zeros(3)
    seed = 7
    for ld in _lds(4096):
        for scale in SCALES:
            for kind in KINDS:
                seed += 1
                worst = np.maximum(worst, _check_case(5, 4096, ld, scale, kind, cuda, seed))
    print(f"\nl2norm dim=4096: fwd {worst[0]:.3e}  inv {worst[1]:.3e}  grad {worst[2]:.3e}  (bound {TOL:.0e})")


@pytest.mark.parametrize("dim", DIMS + (4096,))
def test_gradient_full_cancellation(cuda, dim):
    """dy parallel to x: dy - u (u . dy) cancels completely; the bound still
    holds (it is relative to ||dy||, not to the vanishing result)."""
    worst = 0.0
    for rows in ((5,) if dim == 4096 else (65, 257)):
        for ld in _lds(dim):
            for scale in SCALES:
                for kind in KINDS:
                    worst = max(worst, _check_case(rows, dim, ld, scale, kind, cuda, dim + rows, parallel=True)[2])
    print(f"\nl2norm dim={dim} dy || x: grad {worst:.3e}  (bound {TOL:.0e})")


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("dim", (7, 128, 129, 384, 4096))
def test_in_place_gradient_equals_out_of_place(cuda, dim):
    rows = 5 if dim == 4096 else 257
    for ld in _lds(dim):
        x, dy = _inputs(rows, dim, 1.0, cuda, dim)
        (_, inv), = hip_ops.l2norm_rows([(x, 20.0)])
        db, dv = _buf(rows, dim, ld, cuda, dy)
        (out,) = hip_ops.l2norm_rows_grad([(x, inv, dv, 20.0)])
        (same,) = hip_ops.l2norm_rows_grad([(x, inv, dv, 20.0, dv)])
        assert same.data_ptr() == dv.data_ptr()
        assert _same_bits(dv, out), (dim, ld)
        assert torch.all(db[:, dim:] == SENTINEL)


@pytest.mark.parametrize("shapes", [((65, 129), (257, 7)), ((5, 4096), (63, 128)), ((64, 384), (1, 1)),
                                    ((0, 16), (63, 64))])
def test_two_jobs_equal_two_single_launches(cuda, shapes):
    """Different rows and dims in one launch (also across the kernel's three
    row-width forms, and beside an empty job): bit for bit two single calls."""
    ops = []
    for i, (rows, dim) in enumerate(shapes):
        g = torch.Generator(device="cpu").manual_seed(31 * rows + dim)
        x = torch.relu(torch.randn(rows, dim, generator=g)).to(cuda)
        dy = torch.randn(rows, dim, generator=g).to(cuda)
        ops.append((x, dy, (1.0, 20.0)[i]))
    pair = hip_ops.l2norm_rows([(x, s) for x, _, s in ops])
    pair_g = hip_ops.l2norm_rows_grad([(x, inv, dy, s) for (x, dy, s), (_, inv) in zip(ops, pair)])
    for (x, dy, s), (y, inv), dx in zip(ops, pair, pair_g):
        (y1, inv1), = hip_ops.l2norm_rows([(x, s)])
        (dx1,) = hip_ops.l2norm_rows_grad([(x, inv1, dy, s)])
        assert _same_bits(y, y1) and _same_bits(inv, inv1) and _same_bits(dx, dx1), shapes


@pytest.mark.parametrize("dim", DIMS)
def test_row_result_independent_of_row_count_and_layout(cuda, dim):
    """The first 63 rows of the 257-row call equal the 63-row call bit for
    bit, whatever the leading dimension (16-byte or scalar accesses)."""
    x, dy = _inputs(257, dim, 1.0, cuda, 5 * dim)
    x[0] = x[1]  # (a live first row)
    (y, inv), = hip_ops.l2norm_rows([(x, 20.0)])
    (dx,) = hip_ops.l2norm_rows_grad([(x, inv, dy, 20.0)])
    for ld in _lds(dim):
        _, xs = _buf(63, dim, ld, cuda, x[:63])
        _, ds = _buf(63, dim, ld, cuda, dy[:63])
        _, ys = _buf(63, dim, ld, cuda)
        (y63, inv63), = hip_ops.l2norm_rows([(xs, 20.0, ys)])
        (dx63,) = hip_ops.l2norm_rows_grad([(xs, inv63, ds, 20.0)])
        assert _same_bits(y63, y[:63]) and _same_bits(inv63, inv[:63]) and _same_bits(dx63, dx[:63]), (dim, ld)


def test_two_runs_identical(cuda):
    x, dy = _inputs(257, 129, 1.0, cuda, 3)
    runs = []
    for _ in range(2):
        (y, inv), = hip_ops.l2norm_rows([(x, 20.0)])
        (dx,) = hip_ops.l2norm_rows_grad([(x, inv, dy, 20.0)])
        runs.append((y, inv, dx))
    for a, b in zip(*runs):
        assert _same_bits(a, b)


def test_wrapper_refuses_bad_operands(cuda):
    x = torch.ones(4, 8, device=cuda)
    with pytest.raises(ValueError):
        hip_ops.l2norm_rows([])
    with pytest.raises(ValueError):
        hip_ops.l2norm_rows([(x, 1.0)] * 3)
    with pytest.raises(ValueError):
        hip_ops.l2norm_rows([(x.cpu(), 1.0)])
    with pytest.raises(TypeError):
        hip_ops.l2norm_rows([(x.double(), 1.0)])
    with pytest.raises(ValueError):
        hip_ops.l2norm_rows([(x.t(), 1.0)])  # no unit column stride
    with pytest.raises(ValueError):
        hip_ops.l2norm_rows([(x, 1.0, torch.empty(4, 9, device=cuda))])
    with pytest.raises(ValueError):
        hip_ops.l2norm_rows_grad([(x, torch.ones(3, device=cuda), x, 1.0)])
    from pkg._native import TTError

    with pytest.raises(TTError):
        hip_ops.l2norm_rows([(x, float("nan"))])
