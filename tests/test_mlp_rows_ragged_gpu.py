"""tt_mlp_rows at ragged widths against the parent commit's output.

The epilogue tile is sized by the workgroup's own columns, a wave skips a
column block that lies wholly past N, and the slim width class (N = 258, 260)
deals its last block's row halves to two waves: none of it may change an
output bit.  The reference is not today's code: tests/golden/
mlp_rows_ragged_parent.json holds the digests the parent commit's library
produced for the same calls (tests/golden/make_mlp_rows_ragged_golden.py).
"""
import pytest

import mlp_ragged_golden as rg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from pkg import _native

    return _native.lib()


@pytest.mark.parametrize("run", rg.RUNS)
@pytest.mark.parametrize("case", rg.CASES + [rg.GROUPED_CASE], ids=lambda c: "x".join(map(str, c)))
def test_rows_equal_parent(cuda, lib, case, run):
    """The whole output buffer (padding columns included) and the column sums
    of a single call, bit for bit."""
    want = rg.recorded()["digests"][rg.key(case, run)]
    buf, cs = rg.run_rows(lib, case, run, cuda)
    assert rg.digest(buf) == want["c"]
    assert (cs is None) == ("colsum" not in want)
    if cs is not None:
        assert rg.digest(cs) == want["colsum"]


@pytest.mark.parametrize("run", rg.RUNS)
@pytest.mark.parametrize("i", range(len(rg.CASES) + 1))
def test_rows_pair_equal_parent(cuda, lib, i, run):
    """The same cases through tt_mlp_rows_pair (each with the case three on in
    the list, so the two problems differ in width class; the grouped case
    with a narrow one): both outputs equal the parent's single calls."""
    cases = rg.CASES + [rg.GROUPED_CASE]
    c0, c1 = cases[i], cases[(i + 3) % len(cases)]
    b0, b1 = rg.run_pair(lib, c0, c1, run, cuda)
    rec = rg.recorded()["digests"]
    assert rg.digest(b0) == rec[rg.key(c0, run)]["c"]
    assert rg.digest(b1) == rec[rg.key(c1, run)]["c"]
