"""GPU: the gradient clipping kernels through hip_ops (tt_grad_sumsq,
tt_grad_clip_apply) against the numpy restatement (grad_clip_ref).

Every call is checked the same way (_check):
- ss per variable: |ss_dev - ss_ref| <= n * 2^-52 * ss_ref, n the variable's
  value count (any order of fp64 additions of non-negative exact products
  stays within (n - 1) * 2^-53; an fp32 accumulation cannot meet it);
- the factor is fp32(c / max(n', c)) for n' the reference's fp32 norm or one
  of its two neighbours;
- every element of every region equals fp32(clamp(g) * f_dev) bit for bit,
  and every other word of the buffers (padding columns, neighbouring columns,
  skipped rows pre-filled with a NaN pattern) keeps its bits.
"""
import numpy as np
import pytest
import torch

import grad_clip_ref as ref
from pkg.modelling import hip_ops

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00ABC  # skipped rows are filled with this quiet NaN
# tt_clip.hip: a region owns at most 256 workgroups of 256 threads, each taking
# 4 chunks of 4 floats per trip, so one trip of the capped grid covers
# 256 * 256 * 4 * 4 = 2^20 floats; a longer region runs the loop's second trip
GRID_CAP_FLOATS = 256 * 256 * 4 * 4
SIZES_1D = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4097]


def _values(rng, n, lo=-20, hi=20):
    return (rng.choice([-1.0, 1.0], n) * np.exp2(rng.uniform(lo, hi, n))).astype(np.float32)


class Region:
    """A [rows, cols] range at column `off` of a [rows, ld] matrix that starts
    `shift` floats into its buffer (shift and off set the 16-byte alignment)."""

    def __init__(self, rng, cuda, rows, cols, var, off=0, extra=0, shift=0, ids=None, values=None, one_d=False):
        ld = (off + cols + 2) | 1 if extra == "odd" else off + cols + extra
        self.rows, self.cols, self.var, self.one_d = rows, cols, var, one_d
        n = shift + rows * ld + 8
        init = _values(rng, n)
        pos = (shift + np.arange(rows)[:, None] * ld + off + np.arange(cols)[None, :]).astype(np.int64)
        if values is not None:
            init[pos] = np.asarray(values, np.float32).reshape(rows, cols)
        self.ids = None if ids is None else np.asarray(ids, np.int32)
        valid = np.ones(rows, bool) if ids is None else self.ids >= 0
        bits = init.view(np.uint32)
        bits[pos[~valid].ravel()] = NAN_BITS
        self.init, self.pos = init, pos[valid].ravel()
        self.flat = torch.as_tensor(init.copy(), device=cuda)
        m = self.flat[shift:shift + rows * ld]
        self.g = m[off:off + cols] if one_d else m.view(rows, ld)[:, off:off + cols]
        self.ids_dev = None if ids is None else torch.as_tensor(self.ids, device=cuda)

    def valid_values(self):
        return self.init[self.pos]

    def arg(self):
        return (self.g, self.ids_dev, self.var)


def _run(regs, num_vars, clipvalue=None, clipnorm=None, gclip=None):
    dev = regs[0].flat.device
    norm = clipnorm is not None or gclip is not None
    sumsq = torch.full((num_vars,), -1.0, dtype=torch.float64, device=dev)
    factor = torch.full((num_vars,), -1.0, dtype=torch.float32, device=dev)
    args = [r.arg() for r in regs]
    if norm:
        hip_ops.grad_sumsq(args, num_vars, clipvalue, sumsq)
    hip_ops.grad_clip_apply(args, num_vars, clipvalue, clipnorm, gclip, sumsq if norm else None, factor)
    return sumsq.cpu().numpy(), factor.cpu().numpy()


def _check(regs, num_vars, clipvalue=None, clipnorm=None, gclip=None):
    """Run one call and check everything the module docstring lists; returns
    (ss_dev, f_dev, ss_ref)."""
    ss_dev, f_dev = _run(regs, num_vars, clipvalue, clipnorm, gclip)
    by_var = [[r.valid_values() for r in regs if r.var == v] for v in range(num_vars)]
    ss_ref = [ref.sumsq(v, clipvalue) for v in by_var]
    norm = clipnorm is not None or gclip is not None
    if norm:
        for v in range(num_vars):
            n = sum(a.size for a in by_var[v])
            assert np.isfinite(ss_dev[v])
            assert abs(ss_dev[v] - ss_ref[v]) <= n * 2.0 ** -52 * ss_ref[v], (v, ss_dev[v], ss_ref[v])
    if clipnorm is not None:
        for v in range(num_vars):
            assert f_dev[v].tobytes() in ref.factor_candidates(ss_ref[v], clipnorm), (v, f_dev[v], ss_ref[v])
    elif gclip is not None:
        total = ref.sumsq([a for v in by_var for a in v], clipvalue)
        cands = ref.factor_candidates(total, gclip)
        for v in range(num_vars):
            assert f_dev[v].tobytes() in cands, (v, f_dev[v], total)
        assert len({f.tobytes() for f in f_dev}) == 1
    else:
        assert all(f == np.float32(1.0) for f in f_dev)
    for r in regs:
        want = r.init.copy()
        want[r.pos] = ref.scaled(r.init[r.pos], clipvalue, f_dev[r.var])
        got = r.flat.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (r.rows, r.cols, r.var)
    return ss_dev, f_dev, ss_ref


MODES = [dict(clipnorm=1.0), dict(gclip=1.0), dict(clipvalue=0.25, clipnorm=1.0), dict(clipvalue=4.0, gclip=3.0),
         dict(clipvalue=0.5)]


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "-".join(m))
def test_one_dim_sizes(cuda, mode):
    rng = np.random.default_rng(1)
    regs = [Region(rng, cuda, 1, n, var=2 * i + s, shift=s, one_d=True)
            for i, n in enumerate(SIZES_1D) for s in (0, 1)]
    _check(regs, len(regs), **mode)


@pytest.mark.parametrize("mode", [dict(clipnorm=1.0), dict(clipvalue=8.0, gclip=1.0)], ids=lambda m: "-".join(m))
def test_second_grid_stride_trip(cuda, mode):
    rng = np.random.default_rng(2)
    n = GRID_CAP_FLOATS + 4097
    regs = [Region(rng, cuda, 1, n, var=0, shift=1, one_d=True, values=_values(rng, n, -3, 3))]
    _, f, _ = _check(regs, 1, **mode)
    assert f[0] < 1.0


# (column offset, ld - off - cols, shift of the matrix in its buffer)
PLACEMENTS = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (2, "odd", 0), (3, 0, 1), (0, 0, 1), (1, 3, 3), (0, "odd", 2)]


@pytest.mark.parametrize("place", PLACEMENTS, ids=lambda p: "off%s-extra%s-shift%s" % p)
def test_two_dim_ranges(cuda, place):
    off, extra, shift = place
    rng = np.random.default_rng(3)
    shapes = [(r, c) for r in (0, 1, 37, 513) for c in (1, 4, 7, 16, 100, 129, 300)]
    regs = [Region(rng, cuda, r, c, var=i, off=off, extra=extra, shift=shift) for i, (r, c) in enumerate(shapes)]
    ss, f, _ = _check(regs, len(regs), clipvalue=2.0 ** 18, clipnorm=2.0)
    for i, (r, c) in enumerate(shapes):
        if r == 0:  # an empty region: no value, no clip
            assert ss[i] == 0.0 and f[i] == np.float32(1.0)
    regs = [Region(rng, cuda, r, c, var=i, off=off, extra=extra, shift=shift) for i, (r, c) in enumerate(shapes)]
    _check(regs, len(regs), gclip=0.5)


@pytest.mark.parametrize("k", [2, 4])
def test_regions_sharing_a_variable(cuda, k):
    rng = np.random.default_rng(4)
    regs = [Region(rng, cuda, 37, 7 + 9 * i, var=0, off=i % 4, extra=i) for i in range(k)]
    regs += [Region(rng, cuda, 5, 16, var=1)]
    _, f, _ = _check(regs, 2, clipnorm=1.0)
    assert f[0] < 1.0
    regs = [Region(rng, cuda, 37, 7 + 9 * i, var=0, off=i % 4, extra=i) for i in range(k)]
    regs += [Region(rng, cuda, 5, 16, var=1)]
    _check(regs, 2, clipvalue=1.0, gclip=1.0)


@pytest.mark.parametrize("count", [33, 70])
def test_many_regions_across_launch_chunks(cuda, count):
    """More regions than one launch carries (32): the global norm spans every
    chunk, and a variable's regions lie in different chunks."""
    rng = np.random.default_rng(5)
    nv = 9

    def build():
        return [Region(rng, cuda, 1 + i % 5, 3 + (7 * i) % 50, var=i % nv, off=i % 4, extra=i % 3, shift=i % 2,
                       values=_values(rng, (1 + i % 5) * (3 + (7 * i) % 50), -4, 4)) for i in range(count)]

    _, f, _ = _check(build(), nv, gclip=1.0)
    assert f[0] < 1.0
    _, f, _ = _check(build(), nv, clipvalue=2.0, clipnorm=0.75)
    assert (f < 1.0).all()


@pytest.mark.parametrize("which", ["scattered", "all_invalid", "none_invalid"])
def test_skipped_rows(cuda, which):
    rng = np.random.default_rng(6)
    rows = 131
    ids = rng.integers(0, 50, rows).astype(np.int32)
    if which == "scattered":
        ids[rng.random(rows) < 0.3] = -1
        ids[0] = ids[rows - 1] = -1
    elif which == "all_invalid":
        ids[:] = -1
    for mode in (dict(clipnorm=1.0), dict(clipvalue=1.0, gclip=2.0)):
        regs = [Region(rng, cuda, rows, 20, var=0, ids=ids), Region(rng, cuda, rows, 7, var=0, off=1, ids=ids),
                Region(rng, cuda, 9, 8, var=1)]
        ss, f, _ = _check(regs, 2, **mode)  # finite ss, skipped rows keep their NaN bits: checked there
        if which == "all_invalid":
            assert ss[0] == 0.0
            if "clipnorm" in mode:
                assert f[0] == np.float32(1.0)


def test_million_elements_of_magnitude_one(cuda):
    rng = np.random.default_rng(7)
    n = 1 << 20
    vals = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    regs = [Region(rng, cuda, 1, n, var=0, one_d=True, values=vals)]
    ss, f, ss_ref = _check(regs, 1, clipnorm=1.0)
    assert f[0] < 1e-2
    # what the bound excludes: an fp32 running sum of these values misses it
    s32 = np.cumsum(np.square(vals), dtype=np.float32)[-1]
    assert abs(float(s32) - ss_ref[0]) > n * 2.0 ** -52 * ss_ref[0]


def test_exact_cases(cuda):
    rng = np.random.default_rng(8)
    # n == c: ss = 25, n = 5, f = 5 / 5 = 1
    r = Region(rng, cuda, 1, 2, var=0, one_d=True, values=[3.0, 4.0])
    ss, f, _ = _check([r], 1, clipnorm=5.0)
    assert ss[0] == 25.0 and f[0] == np.float32(1.0)
    assert np.array_equal(r.flat.cpu().numpy().view(np.uint32), r.init.view(np.uint32))
    # n < c: no bit changes (denormals, -0.0 and huge values among them)
    vals = _values(rng, 37 * 9).reshape(37, 9)
    vals[0, :4] = [-0.0, 0.0, 1e-42, -1e-45]
    r = Region(rng, cuda, 37, 9, var=0, off=1, extra=2, values=vals)
    _, f, _ = _check([r], 1, clipnorm=1e30)
    assert f[0] == np.float32(1.0)
    assert np.array_equal(r.flat.cpu().numpy().view(np.uint32), r.init.view(np.uint32))
    r = Region(rng, cuda, 37, 9, var=0, off=1, extra=2, values=vals)
    _, f, _ = _check([r], 1, clipvalue=3e38, gclip=1e30)
    assert np.array_equal(r.flat.cpu().numpy().view(np.uint32), r.init.view(np.uint32))
    # an all-zero gradient: f = 1, no 0 / 0
    for mode in (dict(clipnorm=1.0), dict(gclip=1.0)):
        r = Region(rng, cuda, 5, 6, var=0, values=np.zeros((5, 6), np.float32))
        ss, f, _ = _check([r], 1, **mode)
        assert ss[0] == 0.0 and f[0] == np.float32(1.0)
        assert not np.isnan(r.flat.cpu().numpy()[r.pos]).any()


def test_clipvalue_alone_equals_np_clip(cuda):
    rng = np.random.default_rng(9)
    regs = [Region(rng, cuda, 37, 129, var=0, off=1, extra=1, values=_values(rng, 37 * 129, -3, 3)),
            Region(rng, cuda, 1, 4097, var=1, one_d=True, shift=1, values=_values(rng, 4097, -3, 3))]
    factor = torch.full((2,), -1.0, dtype=torch.float32, device=cuda)
    hip_ops.grad_clip_apply([r.arg() for r in regs], 2, 0.5, None, None, None, factor)  # no sumsq, no norm launch
    assert factor.cpu().tolist() == [1.0, 1.0]
    for r in regs:
        want = r.init.copy()
        want[r.pos] = np.clip(r.init[r.pos], np.float32(-0.5), np.float32(0.5))
        assert np.array_equal(r.flat.cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert (np.abs(want[r.pos]) == 0.5).any() and (np.abs(want[r.pos]) < 0.5).any()


def test_alignment_and_rerun_give_equal_bits(cuda):
    rng = np.random.default_rng(10)
    vals = _values(rng, 513 * 100).reshape(513, 100)
    ids = rng.integers(0, 9, 513).astype(np.int32)
    ids[::7] = -1
    outs = []
    for off, extra, shift in [(0, 0, 0), (0, 0, 0), (1, 0, 0), (0, 1, 2), (3, "odd", 1), (0, 28, 0)]:
        regs = [Region(rng, cuda, 513, 100, var=0, off=off, extra=extra, shift=shift, ids=ids, values=vals),
                Region(rng, cuda, 1, 4097, var=1, one_d=True, shift=shift, values=vals.ravel()[:4097])]
        ss, f, _ = _check(regs, 2, clipvalue=2.0 ** 10, clipnorm=1.0)
        outs.append((ss.tobytes(), f.tobytes(), regs[0].flat.cpu().numpy()[regs[0].pos].tobytes()))
    assert all(o == outs[0] for o in outs)


def test_norm_after_a_triggering_clip(cuda):
    rng = np.random.default_rng(11)
    for c, mode in ((1.0, "clipnorm"), (0.125, "gclip")):
        regs = [Region(rng, cuda, 37, 100, var=0, off=2, extra=1, values=_values(rng, 3700, -2, 6)),
                Region(rng, cuda, 1, 4097, var=1, one_d=True, values=_values(rng, 4097, -2, 6))]
        _, f, _ = _check(regs, 2, **{mode: c})
        assert (f < 1.0).all()
        after = [r.flat.cpu().numpy()[r.pos] for r in regs]
        norms = [np.sqrt(ref.sumsq([a])) for a in after] if mode == "clipnorm" else [np.sqrt(ref.sumsq(after))]
        # one rounding per element plus the factor's rounding
        assert all(n <= c * (1 + 2.0 ** -21) for n in norms), norms


def test_argument_errors(cuda):
    from pkg import _native

    g = torch.zeros(8, dtype=torch.float32, device=cuda)
    ss = torch.zeros(1, dtype=torch.float64, device=cuda)
    with pytest.raises(ValueError):
        hip_ops.grad_sumsq([(g, None, 1)], 1, None, ss)  # var outside range
    with pytest.raises(ValueError):
        hip_ops.grad_clip_apply([(g, None, 0)], 1, None, 1.0, None, None, None)  # a norm without sumsq
    with pytest.raises(_native.TTError):
        hip_ops.grad_clip_apply([(g, None, 0)], 1, None, 1.0, 1.0, ss, None)  # both norms
    assert "both" in _native.lib().tt_last_error().decode()
