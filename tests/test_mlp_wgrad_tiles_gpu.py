"""tt_mlp_wgrad's output tiles: the wide forms (128 x 128 with
TT_WGRAD_TILE=128; unset, 128 x 64 for masked problems and 64 x 128 otherwise)
are bit-identical to the 64 x 64 form (TT_WGRAD_TILE=64, read at every call)
through every entry (tt_mlp_wgrad, _pair, _adagrad), every form reproduces
the recorded output digests of the stand-alone 64 x 64 kernel it replaced,
holds the project's fp32-faithful bound against torch fp64, and leaves the
split counts alone.

The shapes are the smallest that reach each edge of the tiling: one row and
one partial tile; a stage boundary with Ka + 1 = 64; Ka + 1 = 128 exactly; one
row / one 4-column group past 128; three row tiles in one split; S = 4 with a
short last split; S = 32 with 6 empty trailing splits (N no multiple of 64,
then both extents just past a tile edge); the C3 layer geometries at S = 16.
"""
import functools

import pytest
import torch

import wgrad_golden
from pkg import _native
from pkg.modelling import hip_ops

SHAPES = [(1, 5, 4), (33, 63, 64), (130, 127, 128), (130, 128, 132), (130, 287, 256), (1000, 37, 64),
          (4099, 64, 100), (4099, 255, 260), (2048, 258, 256), (2048, 256, 128)]
# the C3 layer-2 geometry is the masked one in training; every shape runs both ways
CASES = [(M, Ka, N, masked) for (M, Ka, N) in SHAPES for masked in (False, True)]


@functools.lru_cache(maxsize=None)
def _inputs(M, Ka, N):
    """One problem's operands (made once, never written): a, g, gmask, scale."""
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(11 + M + 3 * Ka + 7 * N)
    ldg = (N + 3) // 4 * 4
    a = torch.randn(M, (Ka + 3) // 4 * 4, generator=gen, device=dev)[:, :Ka]
    g = torch.randn(M, ldg, generator=gen, device=dev)[:, :N]
    gm = torch.randn(M, ldg, generator=gen, device=dev)[:, :N]
    return a, g, gm, torch.full((1,), 1.5, device=dev)


@functools.lru_cache(maxsize=None)
def _ref64(M, Ka, N, masked):
    a, g, gm, _ = _inputs(M, Ka, N)
    gd = g.double() * ((gm > 0).double() * 1.5 if masked else 1.0)
    return torch.cat([a.double(), torch.ones(M, 1, dtype=torch.float64, device=a.device)], 1).t() @ gd


def _wgrad(M, Ka, N, masked, **kw):
    a, g, gm, s = _inputs(M, Ka, N)
    out = torch.full((Ka + 1, N), float("nan"), device=a.device)
    hip_ops.mlp_wgrad(a, g, out, gmask=gm if masked else None, scale=s if masked else None, **kw)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("M,Ka,N,masked", CASES)
def test_wide_tile_bit_identical_to_64(cuda, monkeypatch, M, Ka, N, masked):
    """Same splits, same 16-row k-steps, same product order: torch.equal."""
    monkeypatch.setenv("TT_WGRAD_TILE", "64")
    ref = _wgrad(M, Ka, N, masked)
    monkeypatch.setenv("TT_WGRAD_TILE", "128")
    wide = _wgrad(M, Ka, N, masked)
    monkeypatch.delenv("TT_WGRAD_TILE")
    default = _wgrad(M, Ka, N, masked)
    assert torch.isfinite(ref).all()
    assert torch.equal(wide, ref)
    assert torch.equal(default, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("M,Ka,N,masked", CASES)
def test_every_tile_matches_recorded_64_digest(cuda, monkeypatch, M, Ka, N, masked):
    """The anchor outside today's code: tests/golden/mlp_wgrad_tile64.json holds
    the SHA-256 of what the stand-alone 64 x 64 kernel wrote for these inputs
    at the last commit that had it (tests/golden/make_wgrad_golden.py); every
    tile setting, "64" included, still writes exactly those bytes."""
    a, g, gm, s = wgrad_golden.device_inputs(M, Ka, N, cuda)
    want = wgrad_golden.recorded()["digests"][wgrad_golden.case_key(M, Ka, N, masked)]
    for tile in wgrad_golden.TILES:
        if tile is None:
            monkeypatch.delenv("TT_WGRAD_TILE", raising=False)
        else:
            monkeypatch.setenv("TT_WGRAD_TILE", tile)
        out = torch.full((Ka + 1, N), float("nan"), device=cuda)
        hip_ops.mlp_wgrad(a, g, out, gmask=gm if masked else None, scale=s if masked else None)
        assert wgrad_golden.digest(out) == want, f"TT_WGRAD_TILE={tile}"


@pytest.mark.gpu
@pytest.mark.parametrize("tile", ["128x64", "64x128"])
@pytest.mark.parametrize("M,Ka,N,masked", [(130, 128, 132, False), (4099, 255, 260, True), (2048, 258, 256, False),
                                           (2048, 256, 128, True)])
def test_other_wide_shapes_bit_identical_to_64(cuda, monkeypatch, tile, M, Ka, N, masked):
    """The wide kernel's 128 x 64 and 64 x 128 forms (measurement knobs)."""
    monkeypatch.setenv("TT_WGRAD_TILE", "64")
    ref = _wgrad(M, Ka, N, masked)
    monkeypatch.setenv("TT_WGRAD_TILE", tile)
    assert torch.equal(_wgrad(M, Ka, N, masked), ref)


@pytest.mark.gpu
def test_unknown_tile_is_an_error(cuda, monkeypatch):
    monkeypatch.setenv("TT_WGRAD_TILE", "96")
    with pytest.raises(Exception, match="TT_WGRAD_TILE"):
        _wgrad(33, 63, 64, False)


@pytest.mark.gpu
@pytest.mark.parametrize("shapes", [((1000, 37, 64), (4099, 64, 100)), ((130, 287, 256), (2048, 258, 256))])
@pytest.mark.parametrize("masked", [False, True])
def test_pair_wide_tile_bit_identical_to_64(cuda, monkeypatch, shapes, masked):
    outs = {}
    for tile in ("64", "128"):
        monkeypatch.setenv("TT_WGRAD_TILE", tile)
        probs = []
        for M, Ka, N in shapes:
            a, g, gm, s = _inputs(M, Ka, N)
            p = dict(a=a, g=g, dwb=torch.full((Ka + 1, N), float("nan"), device=cuda))
            if masked:
                p.update(gmask=gm, scale=s)
            probs.append(p)
        hip_ops.mlp_wgrad_pair(probs)
        outs[tile] = [p["dwb"] for p in probs]
    for (M, Ka, N), w, r in zip(shapes, outs["128"], outs["64"]):
        assert torch.isfinite(r).all()
        assert torch.equal(w, r)
        assert torch.equal(w, _wgrad(M, Ka, N, masked))  # still tile "128": the pair equals the single launch


@pytest.mark.gpu
def test_adagrad_entry_wide_tile_bit_identical_to_64(cuda, monkeypatch):
    M, Ka, N = 2048, 258, 256
    gen = torch.Generator(device=cuda)
    gen.manual_seed(5)
    param0 = torch.randn(Ka + 1, N, generator=gen, device=cuda)
    accum0 = torch.rand(Ka + 1, N, generator=gen, device=cuda) + 0.1
    res = {}
    for tile in ("64", "128"):
        monkeypatch.setenv("TT_WGRAD_TILE", tile)
        param, accum = param0.clone(), accum0.clone()
        dwb = _wgrad(M, Ka, N, False, adagrad=(param, accum, 0.05, 1e-7))
        res[tile] = (dwb, param, accum)
    for w, r in zip(res["128"], res["64"]):
        assert torch.isfinite(r).all()
        assert torch.equal(w, r)
    assert not torch.equal(res["128"][1], param0)


@pytest.mark.gpu
@pytest.mark.parametrize("M,Ka,N,masked", CASES)
def test_wide_tile_vs_torch_fp64(cuda, monkeypatch, M, Ka, N, masked):
    """The bound of test_mlp_wgrad_vs_torch_fp64 (2e-5 relative in norm), and
    two runs bit-equal."""
    monkeypatch.setenv("TT_WGRAD_TILE", "128")
    out = _wgrad(M, Ka, N, masked)
    ref = _ref64(M, Ka, N, masked)
    assert torch.isfinite(out).all()
    err = float((out.double() - ref).norm() / ref.norm())
    print(f"wide tile ({M}, {Ka}, {N}) masked={masked}: rel {err:.3e}")
    assert err < 2e-5
    assert torch.equal(out, _wgrad(M, Ka, N, masked))


def test_wgrad_workspace_size_unchanged():
    """The split counts did not move with the tile: S * (Ka + 1) * N * 4 bytes."""
    lib = _native.lib()
    assert lib.tt_mlp_wgrad_workspace_size(16384, 258, 256) == 8486912
    assert lib.tt_mlp_wgrad_workspace_size(16384, 256, 128) == 8421376
    assert lib.tt_mlp_wgrad_workspace_size(16384, 212, 256) == 13959168
