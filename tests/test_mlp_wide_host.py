"""CPU: Dense layers wider than 384.  tt_mlp_rows validates N up to 4096 on
the host (a problem of no rows returns before any stream use, so no kernel
is launched by these tests), and Tower builds stacks up to that width while
the bare DenseStack constructor keeps its 384 default."""
import ctypes

import pytest
import torch

from pkg import _native, dtypes
from pkg.modelling.models.tower import DenseStack, Tower
from pkg.schema.features import Feature, FeatureFamily

CPU = torch.device("cpu")


def _rows_no_rows(lib, K, N):
    """tt_mlp_rows on M = 0 rows with dummy non-NULL pointers."""
    one = ctypes.c_void_p(16)
    return lib.tt_mlp_rows(one, (K + 3) // 4 * 4, None, 0, None, 0, K, one, N, None, 0, None, 0, one,
                           (N + 3) // 4 * 4, None, None, 0, None)


@pytest.mark.parametrize("N", [384, 385, 512, 772, 4096])
def test_mlp_rows_accepts_widths_to_4096(N):
    lib = _native.lib()
    assert _rows_no_rows(lib, 64, N) == _native.TT_OK, lib.tt_last_error().decode()


def test_mlp_rows_refuses_4097_naming_the_bound():
    lib = _native.lib()
    rc = _rows_no_rows(lib, 64, 4097)
    assert rc == _native.TT_ERR_UNSUPPORTED
    msg = lib.tt_last_error().decode()
    assert "4096" in msg and "4097" in msg
    with pytest.raises(_native.TTError):
        _native.check(rc)


def test_mlp_rows_pair_validates_both_widths():
    lib = _native.lib()
    arr = (_native.MlpRowsProblem * 2)()
    for q, n in zip(arr, (512, 128)):
        q.A, q.lda, q.M, q.K, q.img, q.N, q.C, q.ldc = 16, 64, 0, 64, 16, n, 16, n
    assert lib.tt_mlp_rows_pair(arr, None) == _native.TT_OK, lib.tt_last_error().decode()
    arr[1].N = arr[1].ldc = 4100
    assert lib.tt_mlp_rows_pair(arr, None) == _native.TT_ERR_UNSUPPORTED
    assert "4096" in lib.tt_last_error().decode()


def _features(n_cat, dim, n_num):
    V = [str(i) for i in range(10)]
    return [Feature(f"num{i}", dtypes.float32, FeatureFamily.QUERY) for i in range(n_num)] + \
           [Feature(f"cat{i}", dtypes.string, FeatureFamily.QUERY, embedding_size=dim, vocab=V) for i in range(n_cat)]


def test_tower_with_512_hidden_layer_constructs():
    gen = torch.Generator()
    gen.manual_seed(0)
    t = Tower(_features(2, 16, 0), 128, hidden_units=[512], device=CPU, generator=gen)
    # (w_off, fan_in, fan_out, b_off): kernel rows then the bias, layer after layer
    assert t.dense.layout == [(0, 32, 512, 32 * 512), (33 * 512, 512, 128, 33 * 512 + 512 * 128)]
    assert t.dense.flat.numel() == 33 * 512 + 513 * 128
    assert t.dense.out_dim == 128
    (w0, b0), (w1, b1) = t.dense.params()
    assert tuple(w0.shape) == (32, 512) and tuple(b0.shape) == (512,)
    assert tuple(w1.shape) == (512, 128) and tuple(b1.shape) == (128,)
    assert 0 < float(w0.detach().abs().max()) <= (6.0 / (32 + 512)) ** 0.5  # glorot_uniform
    assert not b0.any() and not b1.any()


def test_tower_with_386_wide_input_constructs():
    gen = torch.Generator()
    gen.manual_seed(1)
    t = Tower(_features(3, 128, 2), 128, hidden_units=[256], device=CPU, generator=gen)
    assert t.input_layer.output_dim == 386
    assert t.dense.layout[0][1:3] == (386, 256)


def test_tower_refuses_widths_over_4096_naming_the_bound():
    with pytest.raises(ValueError, match="4096"):
        Tower(_features(1, 16, 0), 128, hidden_units=[4097], device=CPU, generator=torch.Generator())


def test_dense_stack_max_width_is_opt_in():
    gen = torch.Generator()
    gen.manual_seed(2)
    st = DenseStack(8, [4096, 4], CPU, gen, max_width=4096)
    assert st.layout[0][1:3] == (8, 4096) and st.layout[1][1:3] == (4096, 4)
    DenseStack(4096, [4], CPU, gen, max_width=4096)
    with pytest.raises(ValueError, match="4096"):
        DenseStack(8, [4097, 4], CPU, gen, max_width=4096)
    with pytest.raises(ValueError, match="4096"):
        DenseStack(4097, [4], CPU, gen, max_width=4096)
    with pytest.raises(ValueError, match="4096"):  # the kernels' bound caps the option itself
        DenseStack(8, [4], CPU, gen, max_width=8192)
    with pytest.raises(ValueError, match="384"):  # the bare constructor keeps its default
        DenseStack(8, [512, 4], CPU, gen)
    with pytest.raises(ValueError, match="384"):
        DenseStack(386, [4], CPU, gen)
