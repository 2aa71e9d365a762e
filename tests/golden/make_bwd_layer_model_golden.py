"""Recorded tests/golden/bwd_layer_model_parent.json: the digests of
tests/bwd_layer_model_golden.py's run() (three graphed train steps of a small
model with the C3 tower widths: losses, dense buffers, tables, accumulators)
at the commit named in the fixture's "commit" field: the last one before
DenseStack's backward issued one tt_mlp_backward_layer launch per layer.

THE RULE.  A run of this script against later code would compare that code
with itself, so the fixture is never regenerated: this script is the record
of how it was made and refuses to overwrite it.

Run on an MI355X in a checkout of that commit with libtt.so built, after
copying this script and tests/bwd_layer_model_golden.py into it (the model
runs on that checkout's package and library):
  python tests/golden/make_bwd_layer_model_golden.py <commit hash> [output path]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd"), os.path.dirname(HERE)]
import torch  # noqa: E402

import bwd_layer_model_golden as bg  # noqa: E402

commit = sys.argv[1]
path = sys.argv[2] if len(sys.argv) > 2 else bg.FIXTURE
if os.path.exists(bg.FIXTURE):
    sys.exit(f"{bg.FIXTURE} exists: it is never regenerated (see this script's docstring)")
dev = torch.device("cuda:0")
digests = bg.run(dev)
assert digests == bg.run(dev), "the steps are not reproducible run to run"
with open(path, "w") as f:
    json.dump({"commit": commit, "inputs": "tests/bwd_layer_model_golden.py: run()",
               "hash": "sha256 of each tensor's bytes", "digests": digests}, f, indent=1)
    f.write("\n")
print("wrote", path)
