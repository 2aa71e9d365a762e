"""tt_mlp_rows after its epilogue mask loads were batched, the dead A
prefetches dropped and the bias load hoisted, and tt_mlp_wgrad_adagrad after
the partial-sum kernel loads its Adagrad operands early: every output byte is
what the kernels wrote before (tests/golden/mlp_rows_parent.json, recorded by
tests/golden/make_mlp_rows_golden.py at the commit it names), and,
independent of that record, within the fp32-faithful bound of
test_kernels_gpu.py (2e-5 relative in norm) of torch fp64.

The cases (tests/mlp_rows_golden.py) cover M in {1, 63, 64, 65, 130, 1000},
K in {16, 64, 128, 200, 258} and N in {4, 100, 128, 132, 256, 258, 384}: K = 64
and 128 put the dead stages right after the first / second stage; N = 132 and
258 store ragged rows; an output pitch that is no multiple of 4 (N = 100 with
ldc = 102, N = 258 with ldc = 258) and N = 258 under a mask take the scalar
path, N = 100 with ldc = 100 the narrowest vector rows (100 % 4 == 0: these
are vector stores, not scalar ones); ldcm != ldc in most; both masks hold
+0.0, -0.0 and negatives; A is the tail of its allocation.
"""
import pytest
import torch

import mlp_rows_golden as mg


@pytest.mark.gpu
@pytest.mark.parametrize("case", mg.ROWS_CASES, ids=lambda c: mg.rows_key(*c))
def test_rows_bit_identical_to_recorded_parent(cuda, case):
    want = mg.recorded()["digests"]
    for run in mg.RUNS:
        buf, cs = mg.run_rows(case, run, cuda)
        got = mg.digest(buf) if cs is None else mg.digest(buf, cs)
        assert got == want[f"{mg.rows_key(*case)}-{run}"], run


@pytest.mark.gpu
@pytest.mark.parametrize("case", mg.ROWS_CASES, ids=lambda c: mg.rows_key(*c))
def test_rows_vs_torch_fp64(cuda, case):
    M, K, N, ldc, dcm = case
    for run in mg.RUNS:
        buf, cs = mg.run_rows(case, run, cuda)
        out = buf[:, :N]
        ref = mg.rows_ref64(case, run, cuda)
        assert torch.isfinite(out).all()
        err = float((out.double() - ref).norm() / ref.norm().clamp_min(1e-30))
        print(f"{mg.rows_key(*case)} {run}: rel {err:.3e}")
        assert err < 2e-5, run
        # columns past N of a vector-stored ragged row are zeros, otherwise untouched
        assert bool(((buf[:, N:] == 0) | (buf[:, N:] == 7.0)).all())
        if cs is not None:  # the column sums of what was written, in workgroup order
            assert torch.allclose(cs.double(), out.double().sum(0), rtol=1e-5,
                                  atol=1e-5 * float(out.abs().sum(0).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", mg.ADAGRAD_CASES, ids=lambda c: mg.adagrad_key(*c))
def test_wgrad_adagrad_bit_identical_to_recorded_parent(cuda, case):
    assert mg.digest(*mg.run_adagrad(case, cuda)) == mg.recorded()["digests"][mg.adagrad_key(*case)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", mg.ADAGRAD_CASES, ids=lambda c: mg.adagrad_key(*c))
def test_wgrad_adagrad_vs_torch_fp64(cuda, case):
    M, Ka, N, masked = case
    a, g, gm, s, param0, accum0 = mg.adagrad_device(case, cuda)
    dwb, param, accum = mg.run_adagrad(case, cuda)
    gd = g.double() * ((gm > 0).double() * float(s) if masked else 1.0)
    ref = torch.cat([a.double(), torch.ones(M, 1, dtype=torch.float64, device=cuda)], 1).t() @ gd
    assert float((dwb.double() - ref).norm() / ref.norm()) < 2e-5
    # the Adagrad step from the kernel's own summed gradient, in fp32 as
    # tt_dense_adagrad does it.  accum: one IEEE multiply and one add, exact
    # on both sides.  param: sqrt and divide may round differently in torch
    # (a few ulp each: 1e-6 of the update), then one rounding of the
    # difference (2^-23 of the parameter).
    acc = accum0 + dwb * dwb
    assert torch.equal(accum, acc)
    upd = (dwb * mg.LR) / (torch.sqrt(acc) + mg.EPS)
    assert bool(((param - (param0 - upd)).abs() <= 1e-6 * upd.abs() + 2.0 ** -23 * param0.abs()).all())
