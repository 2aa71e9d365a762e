"""CPU: the coefficient table behind Adam's device step clock.

tt_adam_coef_len / tt_adam_coef_fill run on the host (libtt loads without a
GPU).  The table must hold, for every step, the very numbers tt_dense_adam and
tt_sparse_adam compute from `step`; oracle.adam_powers with the two
association orders of oracle.dense_adam and oracle.sparse_adam restates them
in numpy fp32.
"""
import numpy as np
import pytest

from oracle import oracle
from pkg import _native

f32 = np.float32
LR = 1e-3
MAX_LEN = 1 << 22


def oracle_pair(lr, beta1, beta2, step):
    """(alpha of oracle.dense_adam, lr_t of oracle.sparse_adam) at `step`."""
    b1p, b2p = oracle.adam_powers(beta1, beta2, step)
    alpha = f32((f32(lr) * np.sqrt(f32(1) - b2p)) / (f32(1) - b1p))
    lr_t = f32(f32(lr) * (np.sqrt(f32(1) - b2p) / (f32(1) - b1p)))
    return alpha, lr_t


def first_saturated_step(beta1, beta2, limit=40000):
    """The search tt_adam_coef_len makes, in numpy fp32: the first step at which
    1 - beta^t == 1 for both betas."""
    t = np.arange(1, limit + 1, dtype=np.float32)
    sat = np.ones(limit, bool)
    for beta in (beta1, beta2):
        with np.errstate(under="ignore"):
            sat &= (f32(1) - np.power(f32(beta), t).astype(np.float32)) == f32(1)
    assert sat.any()
    first = int(np.argmax(sat))
    assert sat[first:].all()  # the powers are monotone: once saturated, always
    return first + 1


def fill(lr, beta1, beta2, length):
    alpha, lr_t = np.full(max(length, 1), np.nan, np.float32), np.full(max(length, 1), np.nan, np.float32)
    rc = _native.lib().tt_adam_coef_fill(lr, beta1, beta2, length, alpha.ctypes.data, lr_t.ctypes.data)
    return rc, alpha, lr_t


def test_exact_beta_table_equals_the_oracle_formulas():
    b1, b2 = 0.5, 0.75
    L = _native.lib().tt_adam_coef_len(b1, b2)
    assert L == 61
    rc, alpha, lr_t = fill(LR, b1, b2, L + 4)  # a table may be filled past L: the pair stays lr
    assert rc == _native.TT_OK
    for t in range(1, L + 5):
        a, l = oracle_pair(LR, b1, b2, t)
        assert alpha[t - 1].tobytes() == a.tobytes(), t
        assert lr_t[t - 1].tobytes() == l.tobytes(), t
    # the two association orders are not the same numbers: the table keeps both
    assert not np.array_equal(alpha[:L], lr_t[:L])


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.75), (0.0, 0.999)])
def test_len_is_the_first_saturated_step(betas):
    b1, b2 = betas
    L = _native.lib().tt_adam_coef_len(b1, b2)
    assert L == first_saturated_step(b1, b2)
    rc, alpha, lr_t = fill(LR, b1, b2, L)
    assert rc == _native.TT_OK
    assert alpha[L - 1] == f32(LR) and lr_t[L - 1] == f32(LR)
    assert alpha[L - 2] != f32(LR) or lr_t[L - 2] != f32(LR)
    assert not np.isnan(alpha).any() and not np.isnan(lr_t).any()


def test_len_known_values():
    L = _native.lib().tt_adam_coef_len
    assert L(0.9, 0.999) == 17321 and L(0.9, 0.9) == 165 and L(0.0, 0.0) == 1 and L(0.0, 0.5) == 25
    assert L(0.9, 0.9999) == 173250  # the fp32 value of beta, not the real-number formula (173278)


@pytest.mark.parametrize("bad", [1.0, -0.1, 1.5, float("nan")])
def test_len_is_zero_for_a_bad_beta(bad):
    L = _native.lib().tt_adam_coef_len
    assert L(bad, 0.999) == 0 and L(0.9, bad) == 0


def test_len_is_zero_when_the_table_would_pass_2_22_entries():
    beta = float(np.nextafter(f32(1), f32(0)))  # 1 - 2^-24: saturates after ~2.9e8 steps
    assert _native.lib().tt_adam_coef_len(0.9, beta) == 0


def test_fill_rejects_bad_arguments():
    for lr in (float("nan"), float("inf"), -float("inf")):
        assert fill(lr, 0.9, 0.999, 4)[0] == _native.TT_ERR_BAD_ARG
    for length in (0, -3):
        assert fill(LR, 0.9, 0.999, length)[0] == _native.TT_ERR_BAD_ARG
    for b1, b2 in ((1.0, 0.999), (0.9, float("nan")), (-0.1, 0.5)):
        assert fill(LR, b1, b2, 4)[0] == _native.TT_ERR_BAD_ARG
    assert _native.lib().tt_adam_coef_fill(LR, 0.9, 0.999, 4, None, None) == _native.TT_ERR_BAD_ARG
    with pytest.raises(_native.TTError):
        _native.check(fill(LR, 0.9, 0.999, 0)[0])


def test_host_validation_of_the_device_entries():
    """No launch: the device entries refuse bad arguments on the host."""
    lib = _native.lib()
    FAKE = 4096
    jobs = (_native.DenseAdamJob * 9)()
    for j in jobs:
        j.param, j.m, j.v, j.grad, j.n = FAKE, FAKE, FAKE, FAKE, 4
    assert lib.tt_dense_adam_many_dev(jobs, 9, 0.9, 0.999, 1e-7, FAKE, None) == _native.TT_ERR_BAD_ARG
    assert lib.tt_dense_adam_many_dev(jobs, 0, 0.9, 0.999, 1e-7, FAKE, None) == _native.TT_ERR_BAD_ARG
    assert lib.tt_dense_adam_many_dev(jobs, 2, 0.9, 0.999, 1e-7, None, None) == _native.TT_ERR_BAD_ARG
    jobs[1].v = None
    assert lib.tt_dense_adam_many_dev(jobs, 2, 0.9, 0.999, 1e-7, FAKE, None) == _native.TT_ERR_BAD_ARG
    assert lib.tt_adam_clock_advance(None, FAKE, FAKE, 4, None) == _native.TT_ERR_BAD_ARG
    assert lib.tt_adam_clock_advance(FAKE, FAKE, None, 4, None) == _native.TT_ERR_BAD_ARG
    assert lib.tt_adam_clock_advance(FAKE, FAKE, FAKE, 0, None) == _native.TT_ERR_BAD_ARG
    t = (_native.SparseTable * 1)()
    t[0].table, t[0].slot0, t[0].slot1 = FAKE, FAKE, FAKE
    t[0].num_rows, t[0].dim, t[0].num_sources = 100, 8, 1
    t[0].ids[0] = FAKE
    assert lib.tt_sparse_adam_dev(t, 1, 4, FAKE, 64, 0.5, 0.75, 1e-7, None, FAKE, 1 << 40, None) == _native.TT_ERR_BAD_ARG
    assert lib.tt_sparse_adam_dev(t, 1, 4, FAKE, 64, 0.5, 0.75, 1e-7, FAKE, FAKE, 16, None) == _native.TT_ERR_WORKSPACE
    t[0].slot1 = None
    assert lib.tt_sparse_adam_dev(t, 1, 4, FAKE, 64, 0.5, 0.75, 1e-7, FAKE, FAKE, 1 << 40, None) == _native.TT_ERR_BAD_ARG
    t[0].slot1, t[0].dim = FAKE, 4097
    assert lib.tt_sparse_adam_dev(t, 1, 4, FAKE, 64, 0.5, 0.75, 1e-7, FAKE, FAKE, 1 << 40, None) == _native.TT_ERR_BAD_ARG
