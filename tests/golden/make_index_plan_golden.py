"""Recorded tests/golden/index_plan_parent.json: tt_bruteforce_workspace_size
for every k in 1..1120 at three shapes, as the library answered at the commit
named in the fixture's "commit" field: the last one before the exact fallback
got its large-k forms (fewer waves and parts where four per-wave lists pass
the LDS limit).  Up to k = 1120 the fallback is launched as before and the
workspace holds the same buffers, so these values must not move;
tests/test_index_edges_host.py asserts that.

THE RULE.  A run of this script against later code would compare that code
with itself, so the fixture is never regenerated: this script is the record
of how it was made and refuses to overwrite it.

Run against a libtt.so built at that commit (host-only calls, no GPU needed):
  python tests/golden/make_index_plan_golden.py <commit hash> <path to libtt.so>
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "index_plan_parent.json")
SHAPES = [(70, 5000, 32), (2048, 105542, 128), (1 << 20, 1000000, 64)]  # (queries, candidates, dim)
K_LAST = 1120

if __name__ == "__main__":
    commit, lib_path = sys.argv[1], sys.argv[2]
    if os.path.exists(FIXTURE):
        sys.exit(f"{FIXTURE} exists: it is never regenerated (see this script's docstring)")
    lib = ctypes.CDLL(lib_path)
    fn = lib.tt_bruteforce_workspace_size
    fn.restype = ctypes.c_size_t
    fn.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    sizes = {}
    for nq, n, dim in SHAPES:
        vals = [int(fn(nq, n, dim, k)) for k in range(1, K_LAST + 1)]
        assert all(v > 0 for v in vals)
        sizes[f"{nq}x{n}x{dim}"] = vals
    with open(FIXTURE, "w") as f:
        json.dump({"commit": commit,
                   "what": "tt_bruteforce_workspace_size(queries, candidates, dim, k) for k = 1..1120; "
                           "key: queries x candidates x dim, entry k - 1",
                   "sizes": sizes}, f)
        f.write("\n")
    print("wrote", FIXTURE)
