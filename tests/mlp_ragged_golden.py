"""Cases, inputs and digests of tests/golden/mlp_rows_ragged_parent.json (what
tt_mlp_rows wrote at ragged widths before a workgroup's epilogue tile was
sized by its own columns and a wave skipped a column block past N), shared by
tests/test_mlp_rows_ragged_gpu.py and
tests/golden/make_mlp_rows_ragged_golden.py that recorded them.

Everything goes through the C ABI of a library handle (bind()), so the
recording script can run the same calls against another build's libtt.so.
Operands are mlp_rows_golden's (integer arithmetic on the element index).

A case is (M, K, N); the output pitch is N rounded up to 4.  Four runs (RUNS):
  plain         C = relu(A W + b)
  plain-epi     C = (cmask > 0) ? A W^T : 0, with the column sums of C
  masked        C = ((amask > 0) ? A s : 0) W^T
  masked-epi    masked, then the cmask and the column sums
Recorded per case and run: the digest of the whole [M, pitch] output buffer
("c") and of the column sums ("colsum", epi runs).  tt_mlp_rows_pair has no
column sums: its C must equal the "c" of the same run.
"""
import ctypes
import functools
import json
import os

import mlp_rows_golden as mg

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_rows_ragged_parent.json")
RUNS = ("plain", "plain-epi", "masked", "masked-epi")
# M = 130: a partial last row block.  K = 258: a fifth, ragged A stage.
# N: 2 and 33 leave waves without a live block, 130 and 258 / 260 a last unit
# with one live block (258, 260: the slim width class), 212 one dead block,
# 384 none; 772 runs in column groups (3 + 2 + 2 units, the last ragged).
CASES = [(M, K, N) for M in (64, 130) for K in (64, 258) for N in (2, 33, 130, 212, 258, 260, 384)]
GROUPED_CASE = (130, 64, 772)

_vp, _i32, _i64, _sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
_PROTOS = {
    "tt_mlp_pack_bytes": (_sz, [_i32, _i32]),
    "tt_mlp_pack": (_i32, [_vp, _i64, _i32, _i32, _i32, _vp, _sz, _vp]),
    "tt_mlp_rows_workspace_size": (_sz, [_i64, _i32]),
    "tt_mlp_rows": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _vp,
                           _vp, _sz, _vp]),
    "tt_mlp_rows_pair": (_i32, [_vp, _vp]),
    "tt_last_error": (ctypes.c_char_p, []),
}


class RowsProblem(ctypes.Structure):
    """tt_mlp_rows_problem (include/tt.h)."""
    _fields_ = [("A", _vp), ("lda", _i64), ("amask", _vp), ("ldam", _i64), ("scale", _vp), ("M", _i64), ("K", _i32),
                ("img", _vp), ("N", _i32), ("bias", _vp), ("relu", _i32), ("cmask", _vp), ("ldcm", _i64), ("C", _vp),
                ("ldc", _i64)]


def bind(handle):
    """Set the prototypes of the calls used here on a ctypes handle of libtt.so."""
    for name, (restype, argtypes) in _PROTOS.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = restype, argtypes
    return handle


def _ok(lib, rc):
    if rc != 0:
        raise RuntimeError((lib.tt_last_error() or b"").decode())


def key(case, run):
    return "{}x{}x{}-{}".format(*case, run)


def _full(case):
    M, K, N = case
    return (M, K, N, (N + 3) // 4 * 4, 0)


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _images(lib, case, dev):
    """(forward image of w, transposed image of wt), packed once per case."""
    import torch

    M, K, N = case
    d = mg.rows_device(_full(case), dev)
    nbytes = lib.tt_mlp_pack_bytes(K, N)
    out = []
    for w, trans in ((d["w"], 0), (d["wt"], 1)):
        img = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _ok(lib, lib.tt_mlp_pack(w.data_ptr(), w.stride(0), K, N, trans, img.data_ptr(), nbytes, _stream()))
        out.append(img)
    return tuple(out)


def problem(lib, case, run, dev, colsum=True):
    """The operands of one run: (tt_mlp_rows_problem, the [M, pitch] output
    buffer, colsum tensor or None); everything the problem points at stays
    alive in the returned problem's `keep`."""
    import torch

    M, K, N = case
    d = mg.rows_device(_full(case), dev)
    fwd, tr = _images(lib, case, dev)
    buf = torch.full((M, (N + 3) // 4 * 4), 7.0, device=dev)
    q = RowsProblem()
    q.A, q.lda, q.M, q.K, q.N = d["a"].data_ptr(), d["a"].stride(0), M, K, N
    q.C, q.ldc = buf.data_ptr(), buf.stride(0)
    q.img = (fwd if run == "plain" else tr).data_ptr()
    if run == "plain":
        q.bias, q.relu = d["bias"].data_ptr(), 1
    if run.startswith("masked"):
        q.amask, q.ldam, q.scale = d["amask"].data_ptr(), d["amask"].stride(0), d["scale"].data_ptr()
    cs = None
    if run.endswith("-epi"):
        q.cmask, q.ldcm = d["cmask"].data_ptr(), d["cmask"].stride(0)
        if colsum:
            cs = torch.full((N,), 7.0, device=dev)
    q.keep = (d, fwd, tr, buf, cs)
    return q, buf, cs


def run_rows(lib, case, run, dev):
    """One tt_mlp_rows call: (output buffer, colsum or None)."""
    import torch

    M, K, N = case
    q, buf, cs = problem(lib, case, run, dev)
    ws = None
    if cs is not None:
        ws = torch.empty(lib.tt_mlp_rows_workspace_size(M, N), dtype=torch.uint8, device=dev)
    _ok(lib, lib.tt_mlp_rows(q.A, q.lda, q.amask, q.ldam, q.scale, M, K, q.img, N, q.bias, q.relu, q.cmask, q.ldcm,
                             q.C, q.ldc, cs.data_ptr() if cs is not None else None,
                             ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0,
                             _stream()))
    return buf, cs


def run_pair(lib, case0, case1, run, dev):
    """One tt_mlp_rows_pair call of the same run of two cases: the two output buffers."""
    arr = (RowsProblem * 2)()
    keep = []
    for i, case in enumerate((case0, case1)):
        q, buf, _ = problem(lib, case, run, dev, colsum=False)
        ctypes.memmove(ctypes.addressof(arr[i]), ctypes.addressof(q), ctypes.sizeof(RowsProblem))
        keep.append((q, buf))
    _ok(lib, lib.tt_mlp_rows_pair(arr, _stream()))
    return keep[0][1], keep[1][1]


def ref64(case, run, dev):
    """torch fp64 of a run's [M, N] output (the recording script's sanity check)."""
    import torch

    d = mg.rows_device(_full(case), dev)
    a = d["a"].double()
    if run == "plain":
        return torch.relu(a @ d["w"].double() + d["bias"].double())
    if run.startswith("masked"):
        a = a * (d["amask"] > 0).double() * mg.SCALE
    ref = a @ d["wt"].double().t()
    return ref * (d["cmask"] > 0).double() if run.endswith("-epi") else ref


digest = mg.digest


@functools.lru_cache(maxsize=None)
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)
