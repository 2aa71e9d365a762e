"""Cases, inputs and digests of tests/golden/mlp_rows_parent.json (what
tt_mlp_rows and tt_mlp_wgrad_adagrad wrote before the tower kernels' epilogue,
prefetch and partial-sum loads were reordered), shared by
tests/test_mlp_rows_epilogue_gpu.py and tests/golden/make_mlp_rows_golden.py
that recorded them.

Operands are integer arithmetic on the element index (wgrad_golden's hash), so
they depend on no RNG implementation and no device.

A rows case is (M, K, N, ldc, dcm): the output pitch, and the epilogue mask's
pitch as ldc + dcm.  Four runs per case (RUNS):
  fwd     C = relu(A W + b)
  amask   C = ((amask > 0) ? A s : 0) W
  cmask   amask, then C := (cmask > 0) ? C : 0
  parts   cmask with the column sums of C (colsum)
A is the tail of its allocation (the kernel's buffer descriptor ends where
the buffer does), rows 16-B aligned.  Both masks carry +0.0, -0.0 and
negatives.  The output is digested over its whole [M, ldc] buffer, padding
columns included.
"""
import functools
import hashlib
import json
import os

import numpy as np

import wgrad_golden

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_rows_parent.json")
SCALE = 0.75
RUNS = ("fwd", "amask", "cmask", "parts")

# Every M in {1, 63, 64, 65, 130, 1000}, K in {16, 64, 128, 200, 258} and N in
# {4, 100, 128, 132, 256, 258, 384}.  K = 64 / 128: the dead prefetch stages
# come right after the first / second stage.  N = 132, 258: ragged stores.
# ldc % 4 != 0 (100 -> 102, 258 -> 258) is the scalar store path whatever the
# mask; N = 258 with a mask is scalar at any pitch; N = 100, ldc = 100 is the
# narrowest vector row.  dcm != 0: ldcm != ldc.
ROWS_CASES = [
    (1, 16, 4, 4, 4), (1, 258, 384, 384, 0), (63, 64, 100, 100, 4), (63, 128, 256, 256, 8),
    (64, 128, 128, 128, 0), (64, 200, 258, 260, 4), (65, 64, 132, 132, 4), (65, 258, 256, 260, 0),
    (65, 128, 384, 388, -4), (130, 16, 256, 256, 4), (130, 200, 100, 102, 2), (130, 128, 258, 258, 2),
    (130, 64, 384, 384, 4), (1000, 128, 256, 256, 4), (1000, 258, 128, 128, 4), (1000, 200, 132, 136, -4),
    (1000, 64, 4, 8, 0), (1000, 16, 384, 384, 0), (1000, 258, 258, 260, 0), (1000, 128, 100, 100, 0),
    (130, 258, 132, 132, 0), (64, 16, 128, 132, 4),
]
# tt_mlp_wgrad_adagrad: (M, Ka, N, masked)
ADAGRAD_CASES = [(65, 16, 4, False), (130, 258, 256, True), (1000, 200, 128, False), (1000, 64, 100, True),
                 (4113, 256, 128, True)]
LR, EPS = 0.05, 1e-7


def _pad4(n):
    return (n + 3) // 4 * 4


def _mask(rows, ld, salt):
    """wgrad_golden values with every 7th element +0.0 and every 7th + 3 -0.0."""
    m = wgrad_golden._values(rows, ld, salt).copy().reshape(-1)
    idx = np.arange(m.size)
    m[idx % 7 == 0] = 0.0
    m[idx % 7 == 3] = -0.0
    return m.reshape(rows, ld)


def rows_key(M, K, N, ldc, dcm):
    return f"{M}x{K}x{N}-ldc{ldc}-ldcm{ldc + dcm}"


def adagrad_key(M, Ka, N, masked):
    return f"adagrad-{M}x{Ka}x{N}{'-masked' if masked else ''}"


def rows_inputs(M, K, N, ldc, dcm):
    """Host operands: a, amask [M, pad4(K)], w [K, N], wt [N, K], bias [N], cmask [M, ldc + dcm]."""
    salt = (M * 1000003 + K * 10007 + N * 101 + ldc) * 8
    lda = _pad4(K)
    w = wgrad_golden._values(K, N, salt + 3) * np.float32(0.25)
    wt = wgrad_golden._values(N, K, salt + 4) * np.float32(0.25)
    return dict(a=wgrad_golden._values(M, lda, salt + 1), amask=_mask(M, lda, salt + 2), w=w, wt=wt,
                bias=wgrad_golden._values(1, N, salt + 5).reshape(N), cmask=_mask(M, ldc + dcm, salt + 6))


def _tail(host, dev):
    """host [M, ld] as the last M * ld elements of a longer device allocation."""
    import torch

    flat = torch.empty(host.size + 64, dtype=torch.float32, device=dev)
    flat[:64] = float("nan")
    flat[64:] = torch.from_numpy(host).to(dev).reshape(-1)
    return flat[64:].view(host.shape)


@functools.lru_cache(maxsize=None)
def rows_device(case, dev):
    """rows_inputs on dev (made once, never written): the [M, K] / [M, N] views and the scale."""
    import torch

    M, K, N, ldc, dcm = case
    h = rows_inputs(*case)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in h.items() if k != "a"}
    d["a"] = _tail(h["a"], dev)[:, :K]
    d["amask"] = d["amask"][:, :K]
    d["cmask"] = d["cmask"][:, :N]
    d["scale"] = torch.full((1,), SCALE, device=dev)
    return d


def run_rows(case, run, dev):
    """One tt_mlp_rows call: (the whole [M, ldc] output buffer, colsum or None)."""
    import torch

    from pkg.modelling import hip_ops

    M, K, N, ldc, dcm = case
    d = rows_device(case, dev)
    buf = torch.full((M, ldc), 7.0, device=dev)
    out = buf[:, :N]
    if run == "fwd":
        hip_ops.mlp_rows(d["a"], hip_ops.mlp_pack(d["w"]), K, N, out, bias=d["bias"], relu=True)
        return buf, None
    img = hip_ops.mlp_pack(d["wt"], trans=True)
    kw = dict(amask=d["amask"], scale=d["scale"])
    cs = None
    if run in ("cmask", "parts"):
        kw["cmask"] = d["cmask"]
    if run == "parts":
        cs = torch.full((N,), 7.0, device=dev)
        kw["colsum"] = cs
    hip_ops.mlp_rows(d["a"], img, K, N, out, **kw)
    return buf, cs


def rows_ref64(case, run, dev):
    """torch fp64 of run_rows' [M, N] output."""
    import torch

    d = rows_device(case, dev)
    a = d["a"].double()
    if run == "fwd":
        return torch.relu(a @ d["w"].double() + d["bias"].double())
    ref = (a * (d["amask"] > 0).double() * SCALE) @ d["wt"].double().t()
    if run != "amask":
        ref = ref * (d["cmask"] > 0).double()
    return ref


@functools.lru_cache(maxsize=None)
def adagrad_device(case, dev):
    import torch

    M, Ka, N, masked = case
    a, g, gm, s = wgrad_golden.device_inputs(M, Ka, N, dev)
    salt = (M * 1000003 + Ka * 10007 + N * 101) * 8
    param = torch.from_numpy(wgrad_golden._values(Ka + 1, N, salt + 5)).to(dev)
    accum = torch.from_numpy(np.abs(wgrad_golden._values(Ka + 1, N, salt + 6))).to(dev)
    return a, g, gm, s, param, accum


def run_adagrad(case, dev):
    """One tt_mlp_wgrad_adagrad call on fresh copies: (dwb, param, accum)."""
    import torch

    from pkg.modelling import hip_ops

    M, Ka, N, masked = case
    a, g, gm, s, param0, accum0 = adagrad_device(case, dev)
    param, accum = param0.clone(), accum0.clone()
    dwb = torch.full((Ka + 1, N), 7.0, device=dev)
    hip_ops.mlp_wgrad(a, g, dwb, gmask=gm if masked else None, scale=s if masked else None,
                      adagrad=(param, accum, LR, EPS))
    return dwb, param, accum


def digest(*tensors):
    """SHA-256 over the row-major little-endian fp32 bytes of the tensors, in order."""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().astype("<f4", copy=False).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)
