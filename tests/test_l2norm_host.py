"""CPU: the cosine-scoring option's host side — the tt_l2norm_rows /
tt_l2norm_rows_grad symbols, their argument validation (no kernel is launched
by any of these calls), the Tower / TwoTowerModel keyword validation and the
export metadata."""
import ctypes
import math

import pytest
import torch

from pkg import _native, dtypes
from pkg.modelling import export
from pkg.modelling.models.tower import Tower
from pkg.modelling.models.two_tower_model import TwoTowerModel
from pkg.schema.features import Feature, FeatureFamily
from test_native_exports import header_functions

NEW = ("tt_l2norm_rows", "tt_l2norm_rows_grad")
P = 4096  # a non-NULL pointer value; nothing dereferences it on the host


def test_symbols_in_header_binding_and_library():
    lib = _native.lib()
    for name in NEW:
        assert name in header_functions()
        assert name in _native.EXPORTED_SYMBOLS
        assert hasattr(lib, name)


def _fwd(**kw):
    j = _native.L2NormJob(x=P, ldx=8, y=P, ldy=8, inv=P, rows=4, dim=8, scale=1.0)
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _grad(**kw):
    j = _native.L2NormGradJob(x=P, ldx=8, inv=P, dy=P, lddy=8, dx=P, lddx=8, rows=4, dim=8, scale=1.0)
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _call(fn_name, jobs, num_jobs=None):
    lib = _native.lib()
    arr_t = _native.L2NormJob if fn_name == "tt_l2norm_rows" else _native.L2NormGradJob
    arr = (arr_t * max(len(jobs), 1))(*jobs)
    rc = getattr(lib, fn_name)(arr, len(jobs) if num_jobs is None else num_jobs, None)
    return rc, lib.tt_last_error().decode()


FWD_BAD = {
    "null_x": dict(x=None), "null_y": dict(y=None), "null_inv": dict(inv=None),
    "dim_0": dict(dim=0), "dim_4097": dict(dim=4097, ldx=4097, ldy=4097),
    "ldx_below_dim": dict(ldx=7), "ldy_below_dim": dict(ldy=7),
    "scale_nan": dict(scale=math.nan), "scale_inf": dict(scale=math.inf), "scale_ninf": dict(scale=-math.inf),
}
GRAD_BAD = {
    "null_x": dict(x=None), "null_inv": dict(inv=None), "null_dy": dict(dy=None), "null_dx": dict(dx=None),
    "dim_0": dict(dim=0), "dim_4097": dict(dim=4097, ldx=4097, lddy=4097, lddx=4097),
    "ldx_below_dim": dict(ldx=7), "lddy_below_dim": dict(lddy=7), "lddx_below_dim": dict(lddx=7),
    "scale_nan": dict(scale=math.nan), "scale_inf": dict(scale=math.inf),
}


@pytest.mark.parametrize("case", sorted(FWD_BAD))
@pytest.mark.parametrize("slot", [0, 1])
def test_forward_bad_arguments(case, slot):
    jobs = [_fwd(), _fwd()]
    jobs[slot] = _fwd(**FWD_BAD[case])
    rc, msg = _call("tt_l2norm_rows", jobs)
    assert rc == _native.TT_ERR_BAD_ARG
    assert "tt_l2norm_rows" in msg and f"job {slot}" in msg


@pytest.mark.parametrize("case", sorted(GRAD_BAD))
@pytest.mark.parametrize("slot", [0, 1])
def test_gradient_bad_arguments(case, slot):
    jobs = [_grad(), _grad()]
    jobs[slot] = _grad(**GRAD_BAD[case])
    rc, msg = _call("tt_l2norm_rows_grad", jobs)
    assert rc == _native.TT_ERR_BAD_ARG
    assert "tt_l2norm_rows_grad" in msg and f"job {slot}" in msg


@pytest.mark.parametrize("fn,mk", [("tt_l2norm_rows", _fwd), ("tt_l2norm_rows_grad", _grad)])
def test_job_count_and_null_jobs(fn, mk):
    for n in (0, 3, -1):
        rc, msg = _call(fn, [mk(), mk(), mk()], num_jobs=n)
        assert rc == _native.TT_ERR_BAD_ARG and "num_jobs" in msg
    rc = getattr(_native.lib(), fn)(None, 1, None)
    assert rc == _native.TT_ERR_BAD_ARG and "NULL" in _native.lib().tt_last_error().decode()
    with pytest.raises(_native.TTError):
        _native.check(rc)


@pytest.mark.parametrize("fn,mk,ptrs", [("tt_l2norm_rows", _fwd, ("x", "y", "inv")),
                                        ("tt_l2norm_rows_grad", _grad, ("x", "inv", "dy", "dx"))])
def test_zero_rows_is_ok_without_a_launch(fn, mk, ptrs):
    """rows == 0: TT_OK and no work for that job (its pointers are not looked
    at: an empty tensor has none); with every job empty nothing is launched,
    so the call succeeds on a host without a GPU."""
    rc, msg = _call(fn, [mk(rows=0, **{p: None for p in ptrs}), mk(rows=0)])
    assert rc == _native.TT_OK and msg == ""
    # ... and an empty job does not excuse a bad one beside it
    rc, _ = _call(fn, [mk(rows=0), mk(dim=0)])
    assert rc == _native.TT_ERR_BAD_ARG


# ---- keyword validation ------------------------------------------------------
def _features():
    V = [str(i) for i in range(20)]
    return ([Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V)],
            [Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=V)])


CPU = torch.device("cpu")


def test_tower_keywords():
    qf, _ = _features()
    with pytest.raises(ValueError, match="output_scale"):
        Tower(qf, 8, [12], CPU, output_scale=20.0)
    with pytest.raises(ValueError, match="finite"):
        Tower(qf, 8, [12], CPU, normalize=True, output_scale=math.inf)
    t = Tower(qf, 8, [12], CPU)
    assert (t.normalize, t.output_scale, t.dense.normalize, t.dense.output_scale) == (False, 1.0, False, 1.0)
    t = Tower(qf, 8, [12], CPU, normalize=True, output_scale=20.0)
    assert (t.normalize, t.output_scale, t.dense.normalize, t.dense.output_scale) == (True, 20.0, True, 20.0)


@pytest.mark.parametrize("temperature", [0.0, -0.05, math.nan, math.inf])
def test_model_refuses_bad_temperature(temperature):
    qf, cf = _features()
    with pytest.raises(ValueError, match="temperature"):
        TwoTowerModel(qf, cf, "art", 8, [12], [12], device=CPU, normalize_embeddings=True, temperature=temperature)


def test_model_refuses_temperature_without_normalisation():
    qf, cf = _features()
    with pytest.raises(ValueError, match="normalize_embeddings"):
        TwoTowerModel(qf, cf, "art", 8, [12], [12], device=CPU, temperature=0.05)


def test_model_keywords_reach_the_towers():
    qf, cf = _features()
    m = TwoTowerModel(qf, cf, "art", 8, [12], [12], device=CPU, normalize_embeddings=True, temperature=0.05)
    assert (m.normalize_embeddings, m.temperature) == (True, 0.05)
    assert (m.query_tower.normalize, m.query_tower.output_scale) == (True, 1.0 / 0.05)
    assert (m.candidate_tower.normalize, m.candidate_tower.output_scale) == (True, 1.0)
    m = TwoTowerModel(qf, cf, "art", 8, [12], [12], device=CPU, normalize_embeddings=True)
    assert m.temperature is None and m.query_tower.output_scale == 1.0 and m.query_tower.normalize
    m = TwoTowerModel(qf, cf, "art", 8, [12], [12], device=CPU)
    assert not m.normalize_embeddings and m.temperature is None
    assert not m.query_tower.normalize and not m.candidate_tower.dense.normalize


# ---- export metadata -----------------------------------------------------------
def test_tower_metadata_round_trip_and_defaults(tmp_path):
    qf, _ = _features()
    t = Tower(qf, 8, [12], CPU, normalize=True, output_scale=20.0)
    meta = export._tower_meta(t)
    assert meta["normalize"] is True and meta["output_scale"] == 20.0
    t.save(str(tmp_path / "tower.pt"))
    r = Tower.load(str(tmp_path / "tower.pt"), CPU)
    assert (r.normalize, r.output_scale, r.dense.normalize, r.dense.output_scale) == (True, 20.0, True, 20.0)
    assert torch.equal(r.dense.flat, t.dense.flat)
    # a metadata dict written before the fields existed
    old = {k: v for k, v in meta.items() if k not in ("normalize", "output_scale")}
    _, tensors, arrays = export._read(str(tmp_path / "tower"))
    r = export._build_tower(old, tensors, arrays, CPU)
    assert (r.normalize, r.output_scale) == (False, 1.0)


def test_two_tower_metadata_round_trip_and_defaults(tmp_path):
    import json

    qf, cf = _features()
    m = TwoTowerModel(qf, cf, "art", 8, [12], [12], device=CPU, normalize_embeddings=True, temperature=0.05)
    export.save_two_tower(m, str(tmp_path / "two_tower"))
    meta = json.load(open(tmp_path / "two_tower.json"))
    assert meta["normalize_embeddings"] is True and meta["temperature"] == 0.05
    r = export.load_two_tower(str(tmp_path / "two_tower"), CPU)
    assert (r.normalize_embeddings, r.temperature) == (True, 0.05)
    assert (r.query_tower.output_scale, r.candidate_tower.output_scale) == (1.0 / 0.05, 1.0)
    assert r.query_tower.normalize and r.candidate_tower.normalize
    # a file written before the fields existed loads with the defaults
    for k in ("normalize_embeddings", "temperature"):
        del meta[k]
    json.dump(meta, open(tmp_path / "two_tower.json", "w"))
    r = export.load_two_tower(str(tmp_path / "two_tower"), CPU)
    assert (r.normalize_embeddings, r.temperature) == (False, None)
    assert not r.query_tower.normalize and r.query_tower.output_scale == 1.0
