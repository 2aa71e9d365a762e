"""Host: a train step's state lives in its TrainStep, not on the model or
the DenseStacks, and the public signatures kept their positional parameters."""
import inspect

import torch

from pkg import dtypes
from pkg.modelling import losses
from pkg.modelling.models import tower
from pkg.modelling.models.tower import DenseStack
from pkg.modelling.models.two_tower_model import TrainStep, TwoTowerModel
from pkg.modelling.optimizer_factory import OptimizerFactory
from pkg.schema.features import Feature, FeatureFamily

MODEL_NAMES = ("_on_tower", "_on_dx", "_dense_done", "_sparse_done", "_ids_ready")
STACK_NAMES = ("fused_adagrad", "fused_applied", "separate_launches", "_prepacked")


def _positional(fn):
    kinds = (inspect.Parameter.POSITIONAL_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD)
    return [p.name for p in inspect.signature(fn).parameters.values() if p.kind in kinds]


def test_no_step_state_on_model_or_stacks():
    V = [str(i) for i in range(20)]
    q = Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=8, vocab=V)
    c = Feature("art", dtypes.string, FeatureFamily.CANDIDATE, embedding_size=8, vocab=V)
    m = TwoTowerModel([q], [c], "art", 8, [16], [16], device=torch.device("cpu"), seed=0)
    g = torch.Generator()
    g.manual_seed(0)
    bare = DenseStack(12, [16, 8], torch.device("cpu"), g)

    def check():
        assert not [n for n in MODEL_NAMES if hasattr(m, n)]
        for st in (bare, m.query_tower.dense, m.candidate_tower.dense):
            assert not [n for n in STACK_NAMES if hasattr(st, n)]
            assert st.images == {}  # a real attribute, filled by the first pack
        assert m.last_step is None

    check()
    m.compile(optimizer=OptimizerFactory.get_optimizer("adagrad", {"learning_rate": 0.05}))
    check()
    step = TrainStep()
    assert step.mode == "plain" and step.on_tower is None and step.on_dx is None and step.ids_ready is None
    assert step.dense_done == set() and step.sparse_done == set() and len(step.towers) == 2
    for ts in step.towers:
        assert ts.adagrad is None and not ts.separate_launches and ts.fused_layers == set() and not ts.packed
    assert step.towers[0].fused_layers is not step.towers[1].fused_layers


def test_public_signatures_keep_their_positional_parameters():
    want = {
        DenseStack.forward_acts: ["self", "x", "flat"],
        DenseStack.backward_acts: ["self", "acts", "flat", "gout", "gscale", "need_input_grad", "on_dx"],
        DenseStack.backward_split: ["self", "acts", "flat", "gout", "gscale", "need_input_grad"],
        DenseStack.prepack_jobs: ["self", "flat"],
        tower.forward_acts_pair: ["stacks", "xs", "flats"],
        tower.backward_acts_pair: ["stacks", "acts", "flats", "gouts", "gscale", "need_input_grad"],
        TwoTowerModel.tower_loss: ["self", "qi", "ci", "logq", "ids", "weights"],
        TwoTowerModel.compute_loss: ["self", "x", "training"],
        losses.towers_inbatch_softmax_xent: ["qi", "ci", "stack_q", "stack_c", "logq", "reduction", "on_tower",
                                             "on_dx", "ids", "weights", "weight_scale", "num_hard_negatives"],
        losses.global_towers_inbatch_softmax_xent: ["qi", "ci", "stack_q", "stack_c", "comm", "logq", "ids",
                                                    "weights", "weight_scale", "num_hard_negatives"],
    }
    for fn, names in want.items():
        assert _positional(fn) == names, fn.__qualname__
    # what the step adds is keyword-only and defaults to None (a bare call is a bare stack's)
    for fn in (DenseStack.forward_acts, DenseStack.backward_acts, DenseStack.backward_split,
               TwoTowerModel.tower_loss, TwoTowerModel.compute_loss, losses.towers_inbatch_softmax_xent):
        p = inspect.signature(fn).parameters["step"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, fn.__qualname__
    p = inspect.signature(tower.forward_acts_pair).parameters["steps"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
