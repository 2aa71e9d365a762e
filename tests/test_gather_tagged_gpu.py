"""tt_gather_tagged against a numpy take.

The kernel gives each request row a sub-wave of tpr = dim / 4 threads (one
float4 each) and a 256-thread block rpb = 256 // tpr rows; where 256 is not a
multiple of tpr (dim 12: tpr 3, dim 516: tpr 129) the block's tail threads
idle.  Request counts sit on both sides of rpb; tags and rows include the
invalid values next to the valid range; `out` is wider than dim and longer
than n, pre-filled with NaN, so a write outside the gathered columns shows.
The argument checks of the entry point are in tests/test_sparse_edges_host.py.
"""
import os
import re

import numpy as np
import pytest
import torch

from pkg import _native
from pkg.modelling import hip_ops

pytestmark = pytest.mark.gpu


def max_tagged():
    src = open(os.path.join(os.path.dirname(_native.__file__), "..", "..", "csrc", "tt_gather.hip")).read()
    return int(re.search(r"constexpr int kMaxTagged = (\d+);", src).group(1))


ROW_COUNTS = (1, 7, 5000)
PAD, TAIL = 4, 3   # columns right of dim, rows below n: never written


@pytest.mark.parametrize("num_tables", [1, 3, max_tagged()])
@pytest.mark.parametrize("dim", [4, 12, 128, 516, 1024])
def test_gather_tagged_equals_take(cuda, dim, num_tables):
    rng = np.random.default_rng(100 * dim + num_tables)
    rows = [ROW_COUNTS[(t + dim) % 3] for t in range(num_tables)]
    tables = [rng.standard_normal((r, dim)).astype(np.float32) for r in rows]
    dev = [torch.as_tensor(t, device=cuda) for t in tables]
    rpb = 256 // (dim // 4)
    for n in sorted({0, 1, rpb - 1, rpb, rpb + 1, 1000}):
        tags = rng.integers(0, num_tables, size=n).astype(np.int32)
        bad = rng.random(n) < 0.1
        tags[bad] = rng.choice(np.array([-1, num_tables], np.int32), size=int(bad.sum()))
        req = np.zeros(n, np.int32)
        for j in range(n):
            nr = rows[tags[j]] if 0 <= tags[j] < num_tables else 7
            req[j] = rng.choice([-1, nr]) if rng.random() < 0.1 else rng.integers(0, nr)
        want = np.zeros((n, dim), np.float32)
        for j in range(n):
            if 0 <= tags[j] < num_tables and 0 <= req[j] < rows[tags[j]]:
                want[j] = np.take(tables[tags[j]], req[j], axis=0)
        out = torch.full((n + TAIL, dim + PAD), float("nan"), device=cuda)
        hip_ops.gather_tagged(dev, torch.as_tensor(tags, device=cuda), torch.as_tensor(req, device=cuda), out)
        got = out.cpu().numpy()
        assert np.array_equal(got[:n, :dim], want), f"n={n}"
        assert np.isnan(got[:n, dim:]).all(), f"n={n}: padding columns written"
        assert np.isnan(got[n:]).all(), f"n={n}: rows past n written"
        if n >= 256:  # the case is not vacuous: valid and invalid requests both occur
            assert (want != 0).any(axis=1).sum() > n // 2 and (want == 0).all(axis=1).sum() > n // 20
