"""tt_mlp_backward_layer (one Dense layer's backward in one launch) against the
three separate calls it replaces: tt_mlp_wgrad(_adagrad) for the weight
gradient, tt_mlp_rows for the input gradient and the partial sums (+ Adagrad)
that the weight-gradient call ends with.  Everything is compared bit for bit.

A chain of two launches and a finish, as DenseStack.backward_acts issues them:
  1. an upper layer's job alone: no input-gradient role, no pending sums
     (both role-absent forms);
  2. the layer under test: its weight-gradient partials, the input-gradient
     GEMM, and the upper layer's sums + Adagrad;
  3. tt_mlp_wgrad_finish: the layer's own sums + Adagrad.
"""
import numpy as np
import pytest
import torch

import mlp_rows_golden as mg
import wgrad_golden

pytestmark = pytest.mark.gpu

# (Ka, N_hidden, N_in): the weight gradient is [Ka + 1, N_hidden]; the input
# gradient multiplies the [M, N_hidden] gradient by a [N_in, N_hidden] weight
# (None: the layer has no input-gradient role).  N_in = 258 is the slim width
# class, 212 a dead last block, 33 leaves waves 2 and 3 without a block.
SHAPES = [(258, 256, None), (256, 128, 258), (212, 256, 212), (130, 96, 33)]
UPPER = (64, 32)  # the upper layer's (Ka, N): its sums ride in launch 2
LR, EPS = 0.05, 1e-7


def _params(Ka, N, salt, dev):
    param = torch.from_numpy(wgrad_golden._values(Ka + 1, N, salt + 5)).to(dev)
    accum = torch.from_numpy(np.abs(wgrad_golden._values(Ka + 1, N, salt + 6))).to(dev)
    return param, accum


@pytest.mark.parametrize("adagrad_epi", [False, True], ids=["plain", "adagrad-cmask"])
@pytest.mark.parametrize("masked", [False, True], ids=["lower", "top"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("M", [130, 2048])
def test_backward_layer_equals_separate_calls(cuda, M, shape, masked, adagrad_epi):
    """masked: the top layer's ReluGrad mask and scale on the weight gradient's
    G loads and on the input gradient's A loads.  adagrad_epi: both jobs carry
    their Adagrad step and the input gradient an epilogue mask."""
    from pkg.modelling import hip_ops

    Ka, Nh, Nin = shape
    a, g, gm, s = wgrad_golden.device_inputs(M, Ka, Nh, cuda)
    ua, ug, ugm, _ = wgrad_golden.device_inputs(M, UPPER[0], UPPER[1], cuda)
    mk = dict(gmask=gm, scale=s) if masked else {}
    umk = dict(gmask=ugm, scale=s) if masked else {}
    rows = None
    if Nin is not None:
        ld = (Nin + 3) // 4 * 4
        salt = (M * 1000003 + Nh * 10007 + Nin * 101) * 8
        wt = torch.from_numpy(wgrad_golden._values(Nin, Nh, salt + 4) * np.float32(0.25)).to(cuda)
        cmask = torch.from_numpy(mg._mask(M, ld, salt + 6)).to(cuda)[:, :Nin]
        rows = dict(a=g, img=hip_ops.mlp_pack(wt, trans=True), k=Nh, n=Nin)
        if masked:
            rows.update(amask=gm, scale=s)
        if adagrad_epi:
            rows["cmask"] = cmask

    def state(Ka_, N_, salt):
        p, acc = _params(Ka_, N_, salt, cuda)
        return torch.full((Ka_ + 1, N_), 7.0, device=cuda), p, acc

    # the separate calls
    r_udwb, r_up, r_uacc = state(*UPPER, 11)
    r_dwb, r_p, r_acc = state(Ka, Nh, 23)
    hip_ops.mlp_wgrad(ua, ug, r_udwb, adagrad=(r_up, r_uacc, LR, EPS) if adagrad_epi else None, **umk)
    r_out = None
    if rows is not None:
        r_out = torch.full((M, (Nin + 3) // 4 * 4), 7.0, device=cuda)
        q = dict(rows)
        hip_ops.mlp_rows(q.pop("a"), q.pop("img"), q.pop("k"), q.pop("n"), r_out[:, :Nin], **q)
    hip_ops.mlp_wgrad(a, g, r_dwb, adagrad=(r_p, r_acc, LR, EPS) if adagrad_epi else None, **mk)

    # the chain of one-launch layers
    f_udwb, f_up, f_uacc = state(*UPPER, 11)
    f_dwb, f_p, f_acc = state(Ka, Nh, 23)
    upper = hip_ops.mlp_wgrad_job(ua, ug, f_udwb, adagrad=(f_up, f_uacc, LR, EPS) if adagrad_epi else None,
                                  tag="test_bwd_layer_1", **umk)
    job = hip_ops.mlp_wgrad_job(a, g, f_dwb, adagrad=(f_p, f_acc, LR, EPS) if adagrad_epi else None,
                                tag="test_bwd_layer_0", **mk)
    hip_ops.mlp_backward_layer(upper)
    f_out = None
    if rows is not None:
        f_out = torch.full((M, (Nin + 3) // 4 * 4), 7.0, device=cuda)
        hip_ops.mlp_backward_layer(job, dict(rows, out=f_out[:, :Nin]), upper)
    else:
        hip_ops.mlp_backward_layer(job, None, upper)
    hip_ops.mlp_wgrad_finish(job)
    torch.cuda.synchronize()

    for name, r, f in (("upper dwb", r_udwb, f_udwb), ("upper param", r_up, f_up), ("upper accum", r_uacc, f_uacc),
                       ("dwb", r_dwb, f_dwb), ("param", r_p, f_p), ("accum", r_acc, f_acc)):
        assert torch.equal(r, f), name
    if rows is not None:
        assert torch.isfinite(r_out[:, :Nin]).all()
        assert torch.equal(r_out, f_out)  # the whole buffer: padding columns too


def test_backward_layer_refuses_shared_partials(cuda):
    """Consecutive layers must not share a partials buffer (the sums of one
    are read while the other's partials are written) and an input gradient
    wider than one workgroup's 384 columns is tt_mlp_rows' to run."""
    from pkg._native import TTError
    from pkg.modelling import hip_ops

    M = 130
    a, g, _, _ = wgrad_golden.device_inputs(M, 64, 32, cuda)
    j0 = hip_ops.mlp_wgrad_job(a, g, torch.empty(65, 32, device=cuda), tag="test_bwd_layer_same")
    j1 = hip_ops.mlp_wgrad_job(a, g, torch.empty(65, 32, device=cuda), tag="test_bwd_layer_same")
    hip_ops.mlp_backward_layer(j0)
    with pytest.raises(TTError):
        hip_ops.mlp_backward_layer(j1, None, j0)
    hip_ops.mlp_wgrad_finish(j0)
    wt = torch.zeros(772, 32, device=cuda)
    wide = dict(a=g, img=hip_ops.mlp_pack(wt, trans=True), k=32, n=772, out=torch.empty(M, 772, device=cuda))
    with pytest.raises(TTError):
        hip_ops.mlp_backward_layer(j0, wide)
    torch.cuda.synchronize()
