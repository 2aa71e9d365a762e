"""The one-launch layer backward at model level: three graphed train steps of
a small model with the C3 tower widths (258 and 212) leave the losses, dense
weights, tables and accumulators the parent commit left
(tests/golden/bwd_layer_model_parent.json, recorded by
tests/golden/make_bwd_layer_model_golden.py)."""
import pytest

import bwd_layer_model_golden as bg

pytestmark = pytest.mark.gpu


def test_graphed_steps_equal_parent(cuda, monkeypatch):
    from pkg.modelling import hip_ops

    calls = []
    real = hip_ops.mlp_backward_layer
    monkeypatch.setattr(hip_ops, "mlp_backward_layer", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = bg.run(cuda)
    assert calls, "the default backward did not take the one-launch path"
    want = bg.recorded()["digests"]
    assert set(got) == set(want)
    for k in sorted(want):
        assert got[k] == want[k], k
