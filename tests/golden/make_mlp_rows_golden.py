"""Recorded tests/golden/mlp_rows_parent.json: one SHA-256 digest per case and
run of tests/mlp_rows_golden.py (tt_mlp_rows: forward with bias + relu, masked
A with scale, masked A + cmask, cmask + column sums; tt_mlp_wgrad_adagrad:
gradient, parameters and accumulator) of what the kernels wrote at the commit
named in the fixture's "commit" field: the last one before the masked
epilogue's loads were batched, the dead A prefetches dropped and the
partial-sum kernel's Adagrad operands loaded early.

THE RULE.  A run of this script against later code would compare that code
with itself, so the fixture is never regenerated: this script is the record
of how it was made and refuses to overwrite it.  If a digest stops matching,
the kernels changed what they compute; the fixture did not.

Run on an MI355X at that commit, libtt.so built:
  python tests/golden/make_mlp_rows_golden.py <commit hash> [output path]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd"), os.path.dirname(HERE)]
import torch  # noqa: E402

import mlp_rows_golden as mg  # noqa: E402

commit = sys.argv[1]
path = sys.argv[2] if len(sys.argv) > 2 else mg.FIXTURE
if os.path.exists(mg.FIXTURE):
    sys.exit(f"{mg.FIXTURE} exists: it is never regenerated (see this script's docstring)")

dev = torch.device("cuda:0")
digests = {}
for case in mg.ROWS_CASES:
    for run in mg.RUNS:
        buf, cs = mg.run_rows(case, run, dev)
        N = case[2]
        assert torch.isfinite(buf[:, :N]).all()
        ref = mg.rows_ref64(case, run, dev)
        err = float((buf[:, :N].double() - ref).norm() / ref.norm().clamp_min(1e-30))
        assert err < 2e-5, (case, run, err)
        key = f"{mg.rows_key(*case)}-{run}"
        digests[key] = mg.digest(buf) if cs is None else mg.digest(buf, cs)
        again, cs2 = mg.run_rows(case, run, dev)
        assert digests[key] == (mg.digest(again) if cs2 is None else mg.digest(again, cs2)), key
        print(key, digests[key], f"{err:.2e}")
for case in mg.ADAGRAD_CASES:
    key = mg.adagrad_key(*case)
    digests[key] = mg.digest(*mg.run_adagrad(case, dev))
    assert digests[key] == mg.digest(*mg.run_adagrad(case, dev)), key
    print(key, digests[key])

with open(path, "w") as f:
    json.dump({"commit": commit, "inputs": "tests/mlp_rows_golden.py: ROWS_CASES x RUNS, ADAGRAD_CASES",
               "hash": "sha256 of the fp32 bytes: the whole [M, ldc] output buffer (then colsum); dwb, param, accum",
               "digests": digests}, f, indent=1)
    f.write("\n")
print("wrote", path)
