"""Inputs and digests of tests/golden/mlp_wgrad_tile64.json (the output of the
retired 64 x 64 tt_mlp_wgrad kernel), shared by the test that checks them and
tests/golden/make_wgrad_golden.py that recorded them.

The operands depend on no RNG implementation and no device: every element's
fp32 bit pattern is integer arithmetic on its index in the padded array (a
32-bit multiplicative hash carried in numpy uint64).
"""
import functools
import hashlib
import json
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_wgrad_tile64.json")
SCALE = 1.5
# TT_WGRAD_TILE values that must all reproduce the recorded digests (None: unset)
TILES = (None, "64", "128", "128x64", "64x128")

_M32 = np.uint64(0xFFFFFFFF)


def _hash32(n, salt):
    """Element index 0 .. n - 1 -> 32 well-mixed bits: multiply / xor-shift rounds
    mod 2^32, the salt xored in after the first (so two salts give unrelated
    streams, not shifted copies of one)."""
    h = np.arange(n, dtype=np.uint64)
    for mul, sh, x in ((0x9E3779B1, 15, salt & 0xFFFFFFFF), (0x85EBCA77, 13, 0), (0xC2B2AE3D, 16, 0)):
        h = (h * np.uint64(mul)) & _M32
        h ^= (h >> np.uint64(sh)) ^ np.uint64(x)
    return h


def _values(rows, ld, salt):
    """[rows, ld] fp32: sign = hash bit 31, exponent 2^-3 .. 2^0 from bits 29-30
    of a second hash, all 23 explicit mantissa bits from the first (so the bf16
    hi / lo split has a full lo part); magnitudes in [0.125, 2)."""
    h = _hash32(rows * ld, salt)
    e = np.uint64(124) + ((_hash32(rows * ld, salt ^ 0x5BD1E995) >> np.uint64(29)) & np.uint64(3))
    bits = (h & np.uint64(0x80000000)) | (e << np.uint64(23)) | (h & np.uint64(0x7FFFFF))
    return bits.astype(np.uint32).view(np.float32).reshape(rows, ld)


def inputs(M, Ka, N):
    """Host operands a, g, gmask with the leading dimension padded to a multiple
    of 4 (the padding is filled too): columns [:Ka] of a, [:N] of g and gmask."""
    salt = (M * 1000003 + Ka * 10007 + N * 101) * 4
    ldg = (N + 3) // 4 * 4
    return _values(M, (Ka + 3) // 4 * 4, salt + 1), _values(M, ldg, salt + 2), _values(M, ldg, salt + 3)


def device_inputs(M, Ka, N, dev):
    """inputs() copied to dev as the [M, Ka] / [M, N] views of the padded arrays, and the scale."""
    import torch

    a, g, gm = (torch.from_numpy(v).to(dev) for v in inputs(M, Ka, N))
    return a[:, :Ka], g[:, :N], gm[:, :N], torch.full((1,), SCALE, device=dev)


def digest(out):
    """SHA-256 over the row-major little-endian fp32 bytes of a [Ka + 1, N] output tensor."""
    return hashlib.sha256(out.detach().cpu().contiguous().numpy().astype("<f4", copy=False).tobytes()).hexdigest()


def case_key(M, Ka, N, masked):
    return f"{M}x{Ka}x{N}{'-masked' if masked else ''}"


@functools.lru_cache(maxsize=None)
def recorded():
    """The fixture: commit, setting and digests[case_key]."""
    with open(FIXTURE) as f:
        return json.load(f)
