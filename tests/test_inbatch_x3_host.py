"""CPU: the fp32-faithful (x3) rows / cols entries validate their arguments
on the host like the bf16 entries, their workspace holds the two residual
planes, and TT_INBATCH_X3 reaches every library call of
losses.global_inbatch_grads and of the no-grad inbatch_softmax_xent (no
kernel is launched by these tests)."""
import ctypes
import re

import pytest
import torch

from pkg import _native
from pkg.modelling import hip_ops, losses


# --------------------------------------------------------------------------- C ABI
def _rows(lib, q, c, dim, ws, ws_bytes, n_rows=4, n_cols=4, pos_offset=0):
    one = ctypes.c_void_p(16)
    return lib.tt_inbatch_xent_rows_x3(q, dim, n_rows, c, dim, n_cols, dim, None, pos_offset, one, one, None, ws,
                                       ws_bytes, None)


def _cols(lib, q, c, dim, ws, ws_bytes, n_rows=4, n_cols=4, pos_offset=0):
    one = ctypes.c_void_p(16)
    return lib.tt_inbatch_xent_cols_x3(q, dim, n_rows, one, None, c, dim, n_cols, dim, None, pos_offset, one, ws,
                                       ws_bytes, None)


@pytest.mark.parametrize("entry", [_rows, _cols])
def test_x3_entries_host_validation(entry):
    lib = _native.lib()
    one = ctypes.c_void_p(16)
    assert entry(lib, None, None, 8, None, 0) == _native.TT_ERR_BAD_ARG
    assert "NULL q/c" in lib.tt_last_error().decode()
    assert entry(lib, None, one, 8, one, 1 << 30) == _native.TT_ERR_BAD_ARG
    assert entry(lib, one, None, 8, one, 1 << 30) == _native.TT_ERR_BAD_ARG
    # dim > 128 is a valid request this build does not implement
    rc = entry(lib, one, one, 256, one, 1 << 30)
    assert rc == _native.TT_ERR_UNSUPPORTED
    with pytest.raises(_native.TTError):
        _native.check(rc)
    # too small a workspace: the message names the required size
    need = lib.tt_inbatch_x3_workspace_size(4, 4, 8)
    assert need > 0
    for ws, nbytes in ((one, need - 1), (one, 0), (None, need)):
        assert entry(lib, one, one, 8, ws, nbytes) == _native.TT_ERR_WORKSPACE
        m = re.search(r"required (\d+)", lib.tt_last_error().decode())
        assert m and int(m.group(1)) == need
    # the bf16 entries' workspace is too small for the residual planes
    assert entry(lib, one, one, 8, one, lib.tt_inbatch_workspace_size(4, 4, 8)) == _native.TT_ERR_WORKSPACE
    # positives outside the other side's extent
    assert entry(lib, one, one, 8, one, 1 << 30, pos_offset=-1) == _native.TT_ERR_BAD_ARG
    assert entry(lib, one, one, 8, one, 1 << 30, pos_offset=1) == _native.TT_ERR_BAD_ARG
    assert "pos_offset" in lib.tt_last_error().decode()


def test_x3_entries_pos_offset_range_is_per_side():
    """rows: n_rows + pos_offset <= n_cols; cols: n_cols + pos_offset <= n_rows
    (a rank's block inside the gathered extent); checked before the workspace."""
    lib = _native.lib()
    one = ctypes.c_void_p(16)
    assert _rows(lib, one, one, 8, one, 0, n_rows=4, n_cols=12, pos_offset=8) == _native.TT_ERR_WORKSPACE
    assert _rows(lib, one, one, 8, one, 0, n_rows=4, n_cols=12, pos_offset=9) == _native.TT_ERR_BAD_ARG
    assert _cols(lib, one, one, 8, one, 0, n_rows=12, n_cols=4, pos_offset=8) == _native.TT_ERR_WORKSPACE
    assert _cols(lib, one, one, 8, one, 0, n_rows=12, n_cols=4, pos_offset=9) == _native.TT_ERR_BAD_ARG


@pytest.mark.parametrize("R,C,E", [(16384, 16384, 128), (100, 200, 128), (80, 320, 37), (1, 1, 16), (520, 2080, 128),
                                   (2080, 520, 64)])
def test_x3_workspace_holds_the_residual_planes(R, C, E):
    lib = _native.lib()
    base = lib.tt_inbatch_workspace_size(R, C, E)
    assert base > 0
    # both operands' bf16 residual planes, unpadded, on top of the bf16 entries' workspace
    assert lib.tt_inbatch_x3_workspace_size(R, C, E) >= base + 2 * (R + C) * E


def test_x3_workspace_size_unsupported_dim_and_bf16_size_unchanged():
    lib = _native.lib()
    assert lib.tt_inbatch_x3_workspace_size(16, 16, 300) == 0
    assert lib.tt_inbatch_x3_workspace_size(0, 16, 64) == 0
    # the bf16 entries' carve is untouched: the value before the x3 form existed
    assert lib.tt_inbatch_workspace_size(16384, 16384, 128) == 42532864


# --------------------------------------------------------------------------- routing
class _Comm:
    def __init__(self, always=False):
        self.world, self.rank = 1, 0
        if always:
            self.always = True

    def all_gather(self, t):
        return t


class _Recorder:
    """Stands in for hip_ops.inbatch_fused / inbatch_rows / inbatch_cols:
    records every call's keywords, returns correctly shaped CPU tensors."""

    def __init__(self):
        self.calls = []

    def fused(self, q, c, logq, **kw):
        self.calls.append(("fused", kw))
        B, E = q.shape
        return torch.zeros(B), torch.zeros(B), torch.zeros(B, E), torch.zeros(B, E)

    def rows(self, q, c, logq, **kw):
        self.calls.append(("rows", kw))
        R, E = q.shape
        return torch.zeros(R), torch.zeros(R), torch.zeros(R, E) if kw.get("want_dq", True) else None

    def cols(self, q, lse, c, logq, **kw):
        self.calls.append(("cols", kw))
        return torch.zeros(c.shape)

    def of(self, name):
        return [kw for n, kw in self.calls if n == name]


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(hip_ops, "inbatch_fused", r.fused)
    monkeypatch.setattr(hip_ops, "inbatch_rows", r.rows)
    monkeypatch.setattr(hip_ops, "inbatch_cols", r.cols)
    monkeypatch.setattr(hip_ops, "loss_sum", lambda row_loss, scale: row_loss.sum() * scale)
    monkeypatch.setattr(losses, "WORLD1_FUSED", True)
    return r


def _qcl():
    g = torch.Generator().manual_seed(0)
    return torch.randn(6, 8, generator=g), torch.randn(6, 8, generator=g), torch.randn(6, generator=g)


def test_flag_reaches_the_world1_fused_branch(rec, monkeypatch):
    monkeypatch.setenv("TT_INBATCH_X3", "1")
    q, c, logq = _qcl()
    row_loss, dq, dc = losses.global_inbatch_grads(q, c, logq, _Comm())
    assert [n for n, _ in rec.calls] == ["fused"]
    assert rec.of("fused")[0].get("x3") is True
    assert row_loss.shape == (6,) and dq.shape == dc.shape == (6, 8)


def test_flag_reaches_rows_and_cols(rec, monkeypatch):
    monkeypatch.setenv("TT_INBATCH_X3", "1")
    q, c, logq = _qcl()
    losses.global_inbatch_grads(q, c, logq, _Comm(always=True))
    assert [n for n, _ in rec.calls] == ["rows", "cols"]
    assert rec.of("rows")[0].get("x3") is True and rec.of("cols")[0].get("x3") is True
    assert rec.of("rows")[0]["pos_offset"] == 0 and rec.of("cols")[0]["pos_offset"] == 0
    assert rec.of("cols")[0]["row_loss"] is not None


@pytest.mark.parametrize("env", [None, "0"])
def test_flag_unset_keeps_bf16_everywhere(rec, monkeypatch, env):
    if env is None:
        monkeypatch.delenv("TT_INBATCH_X3", raising=False)
    else:
        monkeypatch.setenv("TT_INBATCH_X3", env)
    q, c, logq = _qcl()
    losses.global_inbatch_grads(q, c, logq, _Comm())
    losses.global_inbatch_grads(q, c, logq, _Comm(always=True))
    losses.inbatch_softmax_xent(q, c, logq)
    assert [n for n, _ in rec.calls] == ["fused", "rows", "cols", "rows"]
    assert all(not kw.get("x3", False) for _, kw in rec.calls)


def test_explicit_argument_overrides_the_flag(rec, monkeypatch):
    q, c, logq = _qcl()
    monkeypatch.setenv("TT_INBATCH_X3", "1")
    losses.global_inbatch_grads(q, c, logq, _Comm(), x3=False)
    losses.global_inbatch_grads(q, c, logq, _Comm(always=True), x3=False)
    assert all(not kw.get("x3", False) for _, kw in rec.calls)
    rec.calls.clear()
    monkeypatch.delenv("TT_INBATCH_X3")
    losses.global_inbatch_grads(q, c, logq, _Comm(), x3=True)
    losses.global_inbatch_grads(q, c, logq, _Comm(always=True), x3=True)
    assert [n for n, _ in rec.calls] == ["fused", "rows", "cols"]
    assert all(kw.get("x3") is True for _, kw in rec.calls)


@pytest.mark.parametrize("env", [None, "1"])
def test_injected_rows_and_cols_get_no_new_keyword(rec, monkeypatch, env):
    if env is None:
        monkeypatch.delenv("TT_INBATCH_X3", raising=False)
    else:
        monkeypatch.setenv("TT_INBATCH_X3", env)
    seen = []

    def rows(q, c, logq, pos_offset=0):  # fixed signatures: an x3 keyword would be a TypeError
        seen.append("rows")
        return torch.zeros(q.shape[0]), torch.zeros(q.shape[0]), torch.zeros(q.shape)

    def cols(q, lse, c, logq, pos_offset=0, row_loss=None):
        seen.append("cols")
        return torch.zeros(c.shape)

    q, c, logq = _qcl()
    losses.global_inbatch_grads(q, c, logq, _Comm(), rows=rows, cols=cols)
    assert seen == ["rows", "cols"] and rec.calls == []


def test_eval_loss_uses_the_training_scores(rec, monkeypatch):
    monkeypatch.setenv("TT_INBATCH_X3", "1")
    q, c, logq = _qcl()
    losses.inbatch_softmax_xent(q, c, logq)
    assert [n for n, _ in rec.calls] == ["rows"]
    kw = rec.of("rows")[0]
    assert kw.get("x3") is True and kw.get("want_dq") is False
