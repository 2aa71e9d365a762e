"""Recorded tests/golden/mlp_wgrad_tile64.json: one SHA-256 digest per case of
tests/test_mlp_wgrad_tiles_gpu.py (its 20 CASES, inputs from
tests/wgrad_golden.py) of what tt_mlp_wgrad wrote under TT_WGRAD_TILE=64.

THE RULE.  The digests are the output of the stand-alone 64 x 64 kernel
(mlp_wgrad_block<MASK>) as it was at the commit named in the fixture's
"commit" field, the last one that had it.  Since then TT_WGRAD_TILE=64 selects
the <MASK, 1, 1> form of the one tile template, so a run of this script against
later code would compare that template with itself.  The fixture is therefore
never regenerated from later code: this script is kept as the record of how it
was made and refuses to overwrite it.  If a digest stops matching, the kernels
changed what they compute; the fixture did not.

In the same run every other TT_WGRAD_TILE setting (unset, 128, 128x64, 64x128)
had to give the digest of "64" for every case, or nothing was written.

Run on an MI355X at that commit, libtt.so built:
  python tests/golden/make_wgrad_golden.py <commit hash> [output path]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hm-retrieval-two-tower_amd"), os.path.dirname(HERE)]
import torch  # noqa: E402

import wgrad_golden  # noqa: E402
from pkg.modelling import hip_ops  # noqa: E402
from test_mlp_wgrad_tiles_gpu import CASES  # noqa: E402

commit = sys.argv[1]
path = sys.argv[2] if len(sys.argv) > 2 else wgrad_golden.FIXTURE
if os.path.exists(wgrad_golden.FIXTURE):
    sys.exit(f"{wgrad_golden.FIXTURE} exists: it is never regenerated (see this script's docstring)")

dev = torch.device("cuda:0")
digests = {}
for M, Ka, N, masked in CASES:
    a, g, gm, s = wgrad_golden.device_inputs(M, Ka, N, dev)
    got = {}
    for tile in wgrad_golden.TILES:
        if tile is None:
            os.environ.pop("TT_WGRAD_TILE", None)
        else:
            os.environ["TT_WGRAD_TILE"] = tile
        out = torch.full((Ka + 1, N), float("nan"), device=dev)
        hip_ops.mlp_wgrad(a, g, out, gmask=gm if masked else None, scale=s if masked else None)
        assert torch.isfinite(out).all()
        got[tile] = wgrad_golden.digest(out)
    key = wgrad_golden.case_key(M, Ka, N, masked)
    print(key, got["64"])
    differ = [t for t in wgrad_golden.TILES if got[t] != got["64"]]
    if differ:
        sys.exit(f"{key}: TT_WGRAD_TILE {differ} differ from 64 at this commit: {got}")
    digests[key] = got["64"]

with open(path, "w") as f:
    json.dump({"commit": commit, "setting": "TT_WGRAD_TILE=64", "kernel": "mlp_wgrad_block<MASK> (64 x 64)",
               "inputs": "tests/wgrad_golden.py: inputs(M, Ka, N), scale 1.5", "hash": "sha256 of the fp32 output bytes",
               "digests": digests}, f, indent=1)
    f.write("\n")
print("wrote", path)
