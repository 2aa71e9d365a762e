"""Recorded tests/golden/mlp_rows_ragged_parent.json: SHA-256 digests of what
tt_mlp_rows wrote for every case and run of tests/mlp_ragged_golden.py (CASES
and GROUPED_CASE x RUNS: the whole output buffer, and the column sums of the
epi runs) with the libtt.so of the commit named in the fixture's "commit"
field: the last one before a workgroup's epilogue tile was sized by its own
columns, a wave skipped the column blocks past N and the slim width class
dealt the last block's row halves to two waves.

THE RULE.  A run of this script against later code would compare that code
with itself, so the fixture is never regenerated: this script is the record
of how it was made and refuses to overwrite it.  If a digest stops matching,
the kernels changed what they compute; the fixture did not.

Run on an MI355X with TT_LIB_PATH naming a libtt.so built at that commit
(the calls go through the C ABI only, so the Python package is not involved):
  TT_LIB_PATH=<libtt.so> python tests/golden/make_mlp_rows_ragged_golden.py <commit hash> [output path]
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE)]
import torch  # noqa: E402

import mlp_ragged_golden as rg  # noqa: E402

commit = sys.argv[1]
path = sys.argv[2] if len(sys.argv) > 2 else rg.FIXTURE
if os.path.exists(rg.FIXTURE):
    sys.exit(f"{rg.FIXTURE} exists: it is never regenerated (see this script's docstring)")
lib = rg.bind(ctypes.CDLL(os.environ["TT_LIB_PATH"], mode=ctypes.RTLD_GLOBAL))

dev = torch.device("cuda:0")
digests = {}
for case in rg.CASES + [rg.GROUPED_CASE]:
    for run in rg.RUNS:
        buf, cs = rg.run_rows(lib, case, run, dev)
        N = case[2]
        ref = rg.ref64(case, run, dev)
        err = float((buf[:, :N].double() - ref).norm() / ref.norm().clamp_min(1e-30))
        assert torch.isfinite(buf[:, :N]).all() and err < 2e-5, (case, run, err)
        rec = {"c": rg.digest(buf)}
        if cs is not None:
            rec["colsum"] = rg.digest(cs)
        again, cs2 = rg.run_rows(lib, case, run, dev)
        assert rec["c"] == rg.digest(again) and (cs is None or rec["colsum"] == rg.digest(cs2)), (case, run)
        digests[rg.key(case, run)] = rec
        print(rg.key(case, run), rec["c"][:16], f"{err:.2e}")

with open(path, "w") as f:
    json.dump({"commit": commit, "inputs": "tests/mlp_ragged_golden.py: (CASES + GROUPED_CASE) x RUNS",
               "hash": "sha256 of the fp32 bytes: c = the whole [M, pitch] output buffer, colsum = the column sums",
               "digests": digests}, f, indent=1)
    f.write("\n")
print("wrote", path)
