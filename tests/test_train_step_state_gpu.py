"""GPU: one train step's state is the step's own (TrainStep / TowerStep).

- a step that fails between building the gather's pack jobs and the towers'
  forward leaves nothing behind: the next forward packs images from the
  current weights, the next step is the step of a model that never failed;
- a loss computed outside train_step applies nothing inside its backward,
  after a normal and after a failed step, whatever mode the steps ran in;
- the merged towers-and-loss node in its global-negatives form, on both sides
  of GLOBAL_TOWER_STREAMS, is the hand-assembled chain bit for bit.
The small two-tower model of tests/test_model_gpu.py, Adagrad, batch sizes 37
(ragged) and 256 (aligned).
"""
import numpy as np
import pytest
import torch

from pkg.modelling import hip_ops, losses
from pkg.modelling.layers.input_layer import InputLayer
from pkg.modelling.models import two_tower_model as ttm
from test_cosine_model_gpu import NAMES, _OneRankAlways, _inputs
from test_model_gpu import _batch, _small_model, _state

pytestmark = pytest.mark.gpu


def _fail_next_gather(monkeypatch):
    """InputLayer.gather_many raises on its next call, then works again."""
    real, failed = InputLayer.gather_many, []

    def gather_many(*args, **kwargs):
        if not failed:
            failed.append(True)
            raise RuntimeError("injected gather failure")
        return real(*args, **kwargs)

    monkeypatch.setattr(InputLayer, "gather_many", staticmethod(gather_many))


def _assert_same_state(a, b, what):
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (what, k)


def _towers_out(m, x):
    q, c = m._split(x)
    return m.query_tower(q), m.candidate_tower(c)


@pytest.mark.parametrize("B", [37, 256])
@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("fused", [False, True])
def test_failed_step_leaves_no_stale_images(cuda, monkeypatch, fused, pair, B):
    """The gather fails after the step built its pack jobs: (a) the towers'
    next forward equals a never-failed twin's bit for bit (it packs its images
    from the current weights; a flag left on the stack made it reuse the
    images of the weights before step 1), (b) so does the next train step."""
    monkeypatch.setattr(losses, "TOWER_PAIR", pair)
    m, t = _small_model(cuda, seed=61, fused=fused), _small_model(cuda, seed=61, fused=fused)
    rng = np.random.default_rng(31)
    x, x2 = _batch(cuda, rng, B, True), _batch(cuda, rng, B, True)
    assert torch.equal(m.train_step(x)["loss"], t.train_step(x)["loss"])
    _fail_next_gather(monkeypatch)
    with pytest.raises(RuntimeError, match="injected gather failure"):
        m.train_step(x2)
    assert not any(ts.packed for ts in m.last_step.towers)  # the failed step never saw its images packed
    _assert_same_state(m, t, "the failed step changed nothing")
    for got, want in zip(_towers_out(m, x), _towers_out(t, x)):  # (a)
        assert torch.equal(got, want)
    assert torch.equal(m.train_step(x2)["loss"], t.train_step(x2)["loss"])  # (b)
    _assert_same_state(m, t, "the step after the failed one")
    assert all(ts.packed for ts in m.last_step.towers)
    m.optimizer.check_status(cuda)
    t.optimizer.check_status(cuda)


def _loss_grads(m, x):
    """compute_loss(training=True).backward() outside any train step: the
    loss and every gradient it leaves (both flat gradients must be set)."""
    for tw in m.towers:
        tw.dense.flat.grad = None
    loss = m.compute_loss(x, training=True)
    loss.backward()
    assert all(tw.dense.flat.grad is not None for tw in m.towers)
    grads = [g for tw in m.towers for g in (tw.dense.flat.grad, tw.input_layer.last_grad)]
    return [loss.detach().clone()] + [g.clone() for g in grads]


@pytest.mark.parametrize("B", [37, 256])
@pytest.mark.parametrize("fused", [False, True])
def test_step_state_does_not_outlive_the_step(cuda, monkeypatch, fused, B):
    """m trains in its in-backward modes (the default dense-early step with
    the Adagrad inside the weight-gradient launches, or fused apply); its twin
    takes the same steps with every such mode off.  A loss and backward
    outside train_step — after a normal step, then after a failed one —
    changes no parameter or accumulator and gives the twin's gradients."""
    m, twin = _small_model(cuda, seed=67, fused=fused), _small_model(cuda, seed=67)
    rng = np.random.default_rng(37)
    x, x2 = _batch(cuda, rng, B, True), _batch(cuda, rng, B, True)
    m.train_step(x)
    with monkeypatch.context() as mp:
        for flag in ("DENSE_EARLY", "FUSED_DENSE_WGRAD", "PACK_WITH_GATHER"):
            mp.setattr(ttm, flag, False)
        twin.train_step(x)
        assert twin.last_step.mode == "plain"
        assert not any(ts.packed or ts.fused_layers for ts in twin.last_step.towers)
        want = _loss_grads(twin, x2)
    assert m.last_step.mode == ("fused" if fused else "dense_early")
    _assert_same_state(m, twin, "one step")
    for when in ("after a normal step", "after a failed step"):
        if when == "after a failed step":
            _fail_next_gather(monkeypatch)
            with pytest.raises(RuntimeError, match="injected gather failure"):
                m.train_step(x2)
        before = _state(m)
        got = _loss_grads(m, x2)
        after = _state(m)
        for k in before:
            assert torch.equal(before[k], after[k]), (when, k)
        assert len(got) == len(want) == 5
        for i, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), (when, i)


@pytest.mark.parametrize("B", [37, 4096])
def test_global_form_is_the_hand_assembled_chain(cuda, monkeypatch, B):
    """global_towers_inbatch_softmax_xent on the rows / cols entries at one
    rank, below (one stream) and at (two streams) GLOBAL_TOWER_STREAMS:
    loss, both input gradients and both flat gradients equal forward_acts,
    global_inbatch_grads, loss_sum, backward_acts issued by hand."""
    monkeypatch.setattr(losses, "GLOBAL_TOWER_STREAMS", 4096)
    assert losses._two_streams(torch.empty(B, 1, device=cuda)) == (B == 4096)
    m = _small_model(cuda, seed=71)
    x = _batch(cuda, np.random.default_rng(41), B, True)
    qi, ci, logq, _ = _inputs(m, x)
    sq, sc = m.query_tower.dense, m.candidate_tower.dense
    qi.requires_grad_(True)
    ci.requires_grad_(True)
    loss = losses.global_towers_inbatch_softmax_xent(qi, ci, sq, sc, _OneRankAlways(), logq)
    loss.backward()
    got = (loss.detach(), sq.flat.grad.clone(), sc.flat.grad.clone(), qi.grad, ci.grad)
    sq.flat.grad = sc.flat.grad = None

    fq, fc = sq.flat.detach(), sc.flat.detach()
    ca, qa = sc.forward_acts(ci.detach(), fc), sq.forward_acts(qi.detach(), fq)
    row_loss, dq, dc = losses.global_inbatch_grads(qa[-1], ca[-1], logq, _OneRankAlways())
    one = torch.ones(1, dtype=torch.float32, device=cuda)
    gci, gfc = sc.backward_acts(ca, fc, dc, one, True)
    gqi, gfq = sq.backward_acts(qa, fq, dq, one, True)
    want = (hip_ops.loss_sum(row_loss, 1.0), gfq, gfc, gqi, gci)
    torch.cuda.synchronize()
    assert torch.isfinite(got[0]) and got[1].abs().max() > 0 and got[4].abs().max() > 0
    for name, g, w in zip(NAMES, got, want):
        assert torch.equal(g, w), (B, name)
