"""CPU: the accidental-hit entries (tt_inbatch_*_hits) are exported, bound and
validate their arguments on the host, their workspaces hold the id vectors,
hip_ops checks the id tensors before anything else, the model's
remove_accidental_hits flag round-trips, and losses.global_inbatch_grads hands
each pass the right id vectors (no kernel is launched by these tests)."""
import ctypes
import json
import os

import pytest
import torch

from pkg import _native, dtypes
from pkg.modelling import hip_ops, losses
from pkg.schema.features import Feature, FeatureFamily

NEW = ("tt_inbatch_hits_workspace_size", "tt_inbatch_xent_rows_hits", "tt_inbatch_xent_cols_hits",
       "tt_inbatch_fused_hits_workspace_size", "tt_inbatch_softmax_xent_hits")


def test_hits_symbols_exported_and_bound():
    lib = _native.lib()
    for name in NEW:
        assert name in _native.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None


def _rows(lib, q, c, dim, rid, cid, x3=0):
    one = ctypes.c_void_p(16)
    return lib.tt_inbatch_xent_rows_hits(q, dim, 4, c, dim, 4, dim, None, 0, rid, cid, x3, one, one, None, one,
                                         1 << 30, None)


def _cols(lib, q, c, dim, rid, cid, x3=0):
    one = ctypes.c_void_p(16)
    return lib.tt_inbatch_xent_cols_hits(q, dim, 4, one, None, c, dim, 4, dim, None, 0, rid, cid, x3, one, one,
                                         1 << 30, None)


def _fused(lib, q, c, dim, rid, cid, x3=0):
    one = ctypes.c_void_p(16)
    return lib.tt_inbatch_softmax_xent_hits(q, dim, c, dim, 4, dim, None, rid and cid, x3, one, one, one, one, 1.0,
                                            None, one, 1 << 30, None)


@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("entry", [_rows, _cols, _fused])
def test_hits_entries_host_validation(entry, x3):
    lib = _native.lib()
    one = ctypes.c_void_p(16)
    assert entry(lib, one, one, 8, None, None, x3) == _native.TT_ERR_BAD_ARG
    assert "ids" in lib.tt_last_error().decode()
    assert entry(lib, one, one, 8, one, None, x3) == _native.TT_ERR_BAD_ARG
    assert entry(lib, None, None, 8, one, one, x3) == _native.TT_ERR_BAD_ARG
    # dim > 128 is a valid request this build does not implement
    assert entry(lib, one, one, 256, one, one, x3) == _native.TT_ERR_UNSUPPORTED


@pytest.mark.parametrize("R,C,E", [(16384, 16384, 128), (100, 200, 128), (80, 320, 37), (1, 1, 16), (2080, 520, 64)])
def test_hits_workspaces_hold_the_id_vectors(R, C, E):
    lib = _native.lib()
    plain = {0: lib.tt_inbatch_workspace_size(R, C, E), 1: lib.tt_inbatch_x3_workspace_size(R, C, E)}
    fused = {0: lib.tt_inbatch_fused_workspace_size(R, E), 1: lib.tt_inbatch_fused_x3_workspace_size(R, E)}
    for x3 in (0, 1):
        assert lib.tt_inbatch_hits_workspace_size(R, C, E, x3) >= plain[x3] + 4 * (R + C)
        assert lib.tt_inbatch_fused_hits_workspace_size(R, E, x3) >= fused[x3] + 4 * R
    assert lib.tt_inbatch_hits_workspace_size(R, C, 300, 0) == 0
    assert lib.tt_inbatch_fused_hits_workspace_size(R, 300, 0) == 0


def test_plain_workspaces_unchanged():
    lib = _native.lib()
    # the values before the hits form existed (the plain entries' carve does not move)
    assert lib.tt_inbatch_workspace_size(16384, 16384, 128) == 42532864


def test_plain_entry_too_small_a_workspace_for_hits():
    lib = _native.lib()
    one = ctypes.c_void_p(16)
    ws = lib.tt_inbatch_workspace_size(4, 4, 8)
    rc = lib.tt_inbatch_xent_rows_hits(one, 8, 4, one, 8, 4, 8, None, 0, one, one, 0, one, one, None, one, ws, None)
    assert rc == _native.TT_ERR_WORKSPACE


# --------------------------------------------------------------------------- hip_ops
def _qc(B=6, E=8):
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, E, generator=g), torch.randn(B, E, generator=g)


def test_hip_ops_checks_the_ids_first():
    """The id checks run before the operands' (which need the GPU), so each
    message names the id tensor."""
    q, c = _qc()
    ok = torch.arange(6, dtype=torch.int32)
    with pytest.raises(TypeError, match="ids must be torch.int32"):
        hip_ops.inbatch_fused(q, c, None, ids=ok.long())
    with pytest.raises(ValueError, match=r"ids must be a contiguous \[6\] int32"):
        hip_ops.inbatch_fused(q, c, None, ids=ok[:5])
    with pytest.raises(ValueError, match="contiguous"):
        hip_ops.inbatch_fused(q, c, None, ids=torch.arange(12, dtype=torch.int32)[::2])
    with pytest.raises(ValueError, match="ids must live on the operands' device"):
        hip_ops.inbatch_fused(q, c, None, ids=torch.empty(6, dtype=torch.int32, device="meta"))
    with pytest.raises(TypeError, match="ids must be a torch.Tensor"):
        hip_ops.inbatch_fused(q, c, None, ids=[0, 1, 2, 3, 4, 5])
    with pytest.raises(ValueError, match="prepped=False"):
        hip_ops.inbatch_fused(q, c, None, ws=torch.empty(1), prepped=True, ids=ok)
    for fn, args in ((hip_ops.inbatch_rows, (q, c[:4], None)),
                     (hip_ops.inbatch_cols, (q, torch.zeros(6), c[:4], None))):
        with pytest.raises(ValueError, match="both or neither"):
            fn(*args, row_ids=ok)
        with pytest.raises(TypeError, match="col_ids must be torch.int32"):
            fn(*args, row_ids=ok, col_ids=ok[:4].float())
        with pytest.raises(ValueError, match=r"col_ids must be a contiguous \[4\]"):
            fn(*args, row_ids=ok, col_ids=ok)
        with pytest.raises(ValueError, match=r"row_ids must be a contiguous \[6\]"):
            fn(*args, row_ids=ok[:4], col_ids=ok[:4])
        with pytest.raises(ValueError, match="row_ids must live on"):
            fn(*args, row_ids=torch.empty(6, dtype=torch.int32, device="meta"), col_ids=ok[:4])


# --------------------------------------------------------------------------- model
def _cpu_model(**kw):
    from pkg.modelling.models.two_tower_model import TwoTowerModel

    q = Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=4, vocab=["a", "b"])
    c = Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=4, vocab=["x", "y", "z"])
    return TwoTowerModel([q], [c], "art", 8, [8], [8], {"x": 0.5, "y": 0.3, "z": 0.2}, device=torch.device("cpu"),
                         seed=0, **kw)


def test_model_flag_constructs_and_round_trips(tmp_path):
    from pkg.modelling.models.two_tower_model import TwoTowerModel

    assert _cpu_model().remove_accidental_hits is False
    m = _cpu_model(remove_accidental_hits=True)
    assert m.remove_accidental_hits is True
    path = str(tmp_path / "model" / "two_tower")
    m.save(path)
    meta = json.load(open(os.path.join(os.path.dirname(path), "two_tower.json")))
    assert meta["remove_accidental_hits"] is True
    back = TwoTowerModel.load(path, device=torch.device("cpu"))
    assert back.remove_accidental_hits is True
    _cpu_model().save(path)
    assert TwoTowerModel.load(path, device=torch.device("cpu")).remove_accidental_hits is False


def test_model_hands_the_candidate_column_to_the_loss():
    x = {"cust": torch.tensor([1, 2, 1], dtype=torch.int32), "art": torch.tensor([3, 1, 3], dtype=torch.int32)}
    assert _cpu_model().candidate_ids(x) is None
    ids = _cpu_model(remove_accidental_hits=True).candidate_ids(x)
    assert ids.dtype == torch.int32 and ids.data_ptr() == x["art"].data_ptr()  # a view, not a copy
    ids = _cpu_model(remove_accidental_hits=True).candidate_ids({"art": [[3], [1], [3]]})
    assert ids.dtype == torch.int32 and ids.tolist() == [3, 1, 3]


def test_create_from_schema_forwards_the_flag():
    from types import SimpleNamespace

    from pkg.modelling.models.two_tower_model import TwoTowerModel

    m = _cpu_model()
    schema = SimpleNamespace(query_features=m.query_features, candidate_features=m.candidate_features,
                             model_config=SimpleNamespace(joint_embedding_size=8, query_tower_units=[8],
                                                          candidate_tower_units=[8]),
                             training_config=SimpleNamespace(candidate_prob_lookup=None))
    got = TwoTowerModel.create_from_schema(schema, "art", device=torch.device("cpu"), remove_accidental_hits=True)
    assert got.remove_accidental_hits is True


# --------------------------------------------------------------------------- routing
class _TwoRanks:
    """Rank `rank` of two: all_gather returns both ranks' blocks, given every
    rank's tensors by shape-and-dtype lookup in `peers`."""

    def __init__(self, rank, blocks):
        self.world, self.rank, self.blocks = 2, rank, blocks

    def all_gather(self, t):
        for mine, other in self.blocks:
            if mine is t:
                return torch.cat([mine, other] if self.rank == 0 else [other, mine])
        raise AssertionError("an unexpected tensor was gathered")


def _masked_rows(q, C, L, pos_offset=0, row_ids=None, col_ids=None):
    """torch restatement of the rows pass with the mask (fp64)."""
    R = q.shape[0]
    S = q.double() @ C.double().T - L.double()[None, :]
    r = torch.arange(R)
    hit = row_ids[:, None] == col_ids[None, :]
    hit[r, r + pos_offset] = False
    S = S.masked_fill(hit, float("-inf"))
    lse = torch.logsumexp(S, 1)
    P = torch.exp(S - lse[:, None])
    P[r, r + pos_offset] -= 1.0
    return lse, lse - S[r, r + pos_offset], P @ C.double()


def _masked_cols(Q, lse, c, logq, pos_offset=0, row_loss=None, row_ids=None, col_ids=None):
    n = c.shape[0]
    S = Q.double() @ c.double().T - logq.double()[None, :]
    j = torch.arange(n)
    hit = row_ids[:, None] == col_ids[None, :]
    hit[j + pos_offset, j] = False
    P = torch.exp(S.masked_fill(hit, float("-inf")) - lse[:, None])
    P[j + pos_offset, j] -= 1.0
    return P.T @ Q.double()


@pytest.mark.parametrize("rank", [0, 1])
def test_global_grads_hand_each_pass_the_right_ids(rank):
    """Two fake ranks of 3 rows each, injected torch rows / cols: the rows
    pass gets (local ids, gathered ids), the cols pass (gathered ids, local
    ids), and the rank's results equal its block of the full-batch masked
    loss."""
    g = torch.Generator().manual_seed(3)
    Q, C = torch.randn(6, 4, generator=g), torch.randn(6, 4, generator=g)
    logq = torch.randn(6, generator=g)
    ids = torch.tensor([5, 2, 5, 5, 2, 9], dtype=torch.int32)
    C[2] = C[0]
    me, other = slice(3 * rank, 3 * rank + 3), slice(3 * (1 - rank), 3 * (1 - rank) + 3)
    q, c, lq, my_ids = Q[me], C[me], logq[me], ids[me].contiguous()
    seen = {}

    def rows(q_, C_, L_, pos_offset=0, row_ids=None, col_ids=None):
        seen["rows"] = (row_ids, col_ids, pos_offset)
        return _masked_rows(q_, C_, L_, pos_offset, row_ids, col_ids)

    # every rank's lse and row_loss, which the real ranks would gather
    lse_full, rl_full, dq_full = _masked_rows(Q, C, logq, 0, ids, ids)
    dc_full = _masked_cols(Q, lse_full, C, logq, 0, None, ids, ids)

    def cols(Q_, lse_, c_, logq_, pos_offset=0, row_loss=None, row_ids=None, col_ids=None):
        seen["cols"] = (row_ids, col_ids, pos_offset)
        return _masked_cols(Q_, lse_, c_, logq_, pos_offset, row_loss, row_ids, col_ids)

    class Comm(_TwoRanks):
        def all_gather(self, t):
            if t.dim() == 2 and t.shape[1] == 2 and t.dtype == torch.float64:  # the stacked [lse, row_loss]
                return torch.stack([lse_full, rl_full], 1)
            return super().all_gather(t)

    comm = Comm(rank, [(q, Q[other]), (c, C[other]), (lq, logq[other]), (my_ids, ids[other])])
    row_loss, dq, dc = losses.global_inbatch_grads(q, c, lq, comm, rows=rows, cols=cols, ids=my_ids)
    assert seen["rows"][0] is my_ids and torch.equal(seen["rows"][1], ids) and seen["rows"][2] == 3 * rank
    assert torch.equal(seen["cols"][0], ids) and seen["cols"][1] is my_ids and seen["cols"][2] == 3 * rank
    torch.testing.assert_close(row_loss, rl_full[me], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dq, dq_full[me], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dc, dc_full[me], rtol=1e-12, atol=1e-12)


def test_world1_fused_branch_gets_the_ids(monkeypatch):
    seen = []

    def fused(q, c, logq, **kw):
        seen.append(kw)
        return torch.zeros(6), torch.zeros(6), torch.zeros(6, 8), torch.zeros(6, 8)

    monkeypatch.setattr(hip_ops, "inbatch_fused", fused)
    monkeypatch.setattr(losses, "WORLD1_FUSED", True)
    q, c = _qc()
    ids = torch.arange(6, dtype=torch.int32)
    comm = type("C", (), {"world": 1, "rank": 0, "all_gather": lambda self, t: t})()
    losses.global_inbatch_grads(q, c, None, comm, ids=ids)
    losses.global_inbatch_grads(q, c, None, comm)
    assert seen[0]["ids"] is ids and seen[1].get("ids") is None


def test_eval_loss_gets_the_ids(monkeypatch):
    seen = []

    def rows(q, c, logq, **kw):
        seen.append(kw)
        return torch.zeros(6), torch.zeros(6), None

    monkeypatch.setattr(hip_ops, "inbatch_rows", rows)
    monkeypatch.setattr(hip_ops, "loss_sum", lambda row_loss, scale: row_loss.sum() * scale)
    q, c = _qc()
    ids = torch.arange(6, dtype=torch.int32)
    losses.InBatchSoftmaxCrossEntropy()(q, c, None, ids)
    assert seen[0]["row_ids"] is ids and seen[0]["col_ids"] is ids and seen[0]["want_dq"] is False
