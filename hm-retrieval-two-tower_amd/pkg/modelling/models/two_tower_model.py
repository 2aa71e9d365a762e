"""TwoTowerModel (mirror of /root/reference/pkg/modelling/models/two_tower_model.py:12-205).

train_step (two_tower_model.py:94-130) on MI355X:
  1. query / candidate InputLayer gathers        tt_gather_multi (both towers + logq, 1 launch)
  2. tower MLPs                                   tt_mlp_rows (bf16x3 MFMA, bias + relu epilogue)
  3. scores + logQ + eye-label CE-SUM + dQ/dC     tt_inbatch_softmax_xent (rows + cols passes,
                                                  bf16 MFMA, fp32 accumulation)
  4. MLP backward                                 tt_mlp_wgrad weight + bias gradients and
                                                  tt_mlp_rows input gradients (ReluGrad fused)
  5. optimizer                                    tt_dense_adagrad + tt_sparse_adagrad (dedup in-kernel)
With normalize_embeddings (opt-in cosine scoring, temperature in the query
side's scale): tt_l2norm_rows on both towers' outputs before 3 and
tt_l2norm_rows_grad on dQ, dC after it, one launch each.
Every launch is stream-ordered with no host synchronisation, so the whole step
can be captured once and replayed as a hipGraph (GraphedTrainStep).
"""
from __future__ import annotations

import functools
import logging
import os
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from pkg import dtypes as _dtypes
from pkg.schema.features import Feature
from pkg.schema.schema import Schema
from pkg.modelling.device import default_device, make_generator
from pkg.modelling.layers.logq_correction import LogQCorrection
from pkg.modelling.losses import (TOWER_C_SCOPE, InBatchSoftmaxCrossEntropy, normalized_outputs,
                                  towers_inbatch_softmax_xent)
from pkg.modelling.models.abstract_keras_model import AbstractKerasModel, TensorSpec
from pkg.modelling import hip_ops
from pkg.modelling.layers.input_layer import InputLayer
from pkg.modelling.models import tower as _tower_mod
from pkg.modelling.models.tower import Tower, TowerStep

logger = logging.getLogger(__name__)

__all__ = ["TwoTowerModel", "GraphedTrainStep", "LOGQ_KEY", "WEIGHT_KEY"]

# Optional batch entry carrying per-example log p(candidate) computed from raw
# ids at encoding time (exact even for ids outside a truncated vocab).
LOGQ_KEY = "__logq__"
# Optional batch entry making the batch a WEIGHTED one: per-example sample
# weights, fp32 [B], normalised to [0, 1] (w / w_max; encode_dataframe's
# sample_weight).  The model's sample_weight_scale holds w_max.
WEIGHT_KEY = "__weight__"
# each tower's dense (MLP) Adagrad step issued inside the backward on that
# tower's stream the moment its weight gradient exists, instead of after the
# join (the embedding update stays one call after the backward)
DENSE_EARLY = os.environ.get("TT_DENSE_EARLY", "1") == "1"
# with DENSE_EARLY: each layer's Adagrad step applied by its weight-gradient
# launches (tt_mlp_wgrad_adagrad: the partial-sum launch updates the layer)
# instead of one dense_adagrad launch per tower after its backward
FUSED_DENSE_WGRAD = os.environ.get("TT_FUSED_DENSE_WGRAD", "1") == "1"
# The towers' MLP weight images packed by the train step's gather launch
# (tt_gather_multi_pack) instead of one pack launch per tower at the start of
# each tower's forward (TT_PACK_WITH_GATHER=0).
PACK_WITH_GATHER = os.environ.get("TT_PACK_WITH_GATHER", "1") == "1"


@dataclass
class TrainStep:
    """The state of ONE train step: made by train_step, handed down as step=
    (compute_loss, tower_loss, the towers-and-loss node and, per tower, the
    DenseStacks), readable afterwards as model.last_step (its callbacks
    dropped).  Nothing of it lives on the model or the stacks, so a step that
    raises leaves nothing behind."""
    mode: str = "plain"    # "plain" | "dense_early" | "fused": what the backward applies (train_step)
    on_tower: Optional[Callable] = None   # on_tower(i, input_grad, flat_grad): tower i's gradients exist
    on_dx: Optional[Callable] = None      # on_dx(i, dx): tower i's input gradient exists (IGRAD_FIRST, fused)
    dense_done: set = field(default_factory=set)    # towers whose dense update the backward applied
    sparse_done: set = field(default_factory=set)   # towers whose embedding update ran at their input gradient
    ids_ready: Optional[torch.cuda.Event] = None    # recorded after the gather: the id sorts wait for it only
    towers: Tuple[TowerStep, TowerStep] = field(default_factory=lambda: (TowerStep(), TowerStep()))


class TwoTowerModel(AbstractKerasModel):
    """
    Two Tower Model class.

    Parameters
    ----------
    query_features: List[Feature]
        Features for the query tower.
    candidate_features: List[Feature]
        Features for the candidate tower.
    candidate_id_col: str
        The column containing the candidate_id.
    joint_embedding_size: int
        Joint embedding size which gets dot product.
    query_tower_units: Optional[List[int]]
        Hidden units for the query tower.
    candidate_tower_units: Optional[List[int]]
        Hidden units for the candidate tower.
    candidate_prob_lookup: Optional[Dict[str, float]]
        If provided, logQ correction is applied before the loss.
    remove_accidental_hits: bool
        Off (the default): the reference's loss, every other column of the
        batch a negative.  On: a column that holds the same candidate as a
        row's own positive (equal encoded candidate_id_col; all
        out-of-vocabulary candidates, id 0, count as one) is no negative of
        that row, in training and in evaluation — a departure from the
        reference's loss (TensorFlow Recommenders' remove_accidental_hits).
    sample_weight_scale: float (attribute, default 1.0)
        A batch carrying WEIGHT_KEY ("__weight__": fp32 [B] in [0, 1]) is a
        weighted batch: its loss is sample_weight_scale * sum_i w_i l_i, in
        training and in evaluation (Keras fit(sample_weight=...), with the
        weights normalised by their maximum and the maximum kept here; fit
        takes it from the dataset).  A batch without the key is unweighted.
    normalize_embeddings: bool
        Off (the default): scores are dot products of the towers' ReLU
        outputs, the reference's.  On: both towers' outputs are L2-normalised
        (a dead, all-zero embedding stays zero and gets no gradient), so a
        score is a cosine in [0, 1] — two launches more per train step
        (tt_l2norm_rows, tt_l2norm_rows_grad), the loss kernels unchanged.
    temperature: Optional[float]
        Softmax temperature T > 0 of the cosine scores (TensorFlow
        Recommenders' Retrieval(temperature=...)); needs normalize_embeddings.
        It is the query tower's output scale 1 / T, so call() returns the
        training logits cos / T (before logQ), an index built from the
        candidate tower and queried through the query tower returns cos / T,
        and the ranking does not depend on T.  None: T = 1.
    num_hard_negatives: Optional[int]
        None (the default): every negative of the batch enters the loss.  A
        positive int K: hard-negative mining (TensorFlow Recommenders'
        Retrieval(num_hard_negatives=K)) — of each row's negatives only the K
        with the largest logits (after temperature, logQ and accidental
        hits) keep their weight, in training and in evaluation, on every
        step path; negatives that tie the K-th logit are all kept.  K at or
        above the batch size is the default loss bit for bit.  Anything but
        a positive int raises ValueError.
    num_sampled_negatives: Optional[int]
        None (the default): the negatives are the batch's other candidates.
        A positive int M: mixed negative sampling (Yang et al. 2020) — every
        TRAINING step scores the B queries against B + M columns, the batch's
        candidates followed by M rows drawn uniformly with replacement, fresh
        on every step, from the catalogue attached with
        set_candidate_catalogue.  The extra columns are negatives of every
        row; their embeddings come from the candidate tower and their
        gradient flows back into it and its tables.  With a
        candidate_prob_lookup the logQ shift of a column holding embedding
        row r is the mixture's, log((B p_r + M / N) / (B + M)), N the
        catalogue size.  Evaluation (compute_loss(training=False)) stays the
        plain in-batch loss.  With remove_accidental_hits a sampled column
        holding a row's own positive is masked for that row; without it such
        a column is a negative (one warning is logged).  Anything but a
        positive int raises ValueError.  Single-device only.
    sampled_negatives_seed: int
        Seed of the sampler (Philox4x32-10 keyed by it, counted by the
        model's device step counter).
    """

    def __init__(self, query_features: List[Feature], candidate_features: List[Feature], candidate_id_col: str,
                 joint_embedding_size: int, query_tower_units: Optional[List[int]] = None,
                 candidate_tower_units: Optional[List[int]] = None,
                 candidate_prob_lookup: Optional[Dict[str, float]] = None,
                 device: Optional[torch.device] = None, seed: Optional[int] = None,
                 fused_optimizer_apply: bool = False, remove_accidental_hits: bool = False,
                 normalize_embeddings: bool = False, temperature: Optional[float] = None,
                 num_hard_negatives: Optional[int] = None, num_sampled_negatives: Optional[int] = None,
                 sampled_negatives_seed: int = 0):
        if num_sampled_negatives is not None and (isinstance(num_sampled_negatives, bool)
                                                  or not isinstance(num_sampled_negatives, (int, np.integer))
                                                  or num_sampled_negatives < 1):
            raise ValueError(f"num_sampled_negatives={num_sampled_negatives!r} must be a positive int or None")
        if isinstance(sampled_negatives_seed, bool) or not isinstance(sampled_negatives_seed, (int, np.integer)):
            raise ValueError(f"sampled_negatives_seed={sampled_negatives_seed!r} must be an int")
        self.num_sampled_negatives = None if num_sampled_negatives is None else int(num_sampled_negatives)
        self.sampled_negatives_seed = int(sampled_negatives_seed)
        self.candidate_catalogue = None
        self._mixed_buffers: Dict[int, torch.Tensor] = {}   # B -> the assembled [F, B + M] candidate words
        self._mixed_logq: Dict[tuple, torch.Tensor] = {}    # (B, M) -> the mixture's logQ per embedding row
        self._mixed_step: Optional[torch.Tensor] = None     # the sampler's step counter (device int64 [1])
        self._mixed_status: Optional[torch.Tensor] = None
        self._mixed_warned = False
        if num_hard_negatives is not None and (isinstance(num_hard_negatives, bool)
                                               or not isinstance(num_hard_negatives, (int, np.integer))
                                               or num_hard_negatives < 1):
            raise ValueError(f"num_hard_negatives={num_hard_negatives!r} must be a positive int or None")
        self.num_hard_negatives = None if num_hard_negatives is None else int(num_hard_negatives)
        self.normalize_embeddings = bool(normalize_embeddings)
        if temperature is not None:
            temperature = float(temperature)
            if not 0.0 < temperature < float("inf"):
                raise ValueError(f"temperature={temperature} must be a positive finite number")
            if not self.normalize_embeddings:
                raise ValueError("temperature needs normalize_embeddings=True (on unbounded dot products it only "
                                 "rescales the top layers)")
        self.temperature = temperature
        self.remove_accidental_hits = bool(remove_accidental_hits)
        self.sample_weight_scale = 1.0
        # apply each tower's Adagrad step inside the backward (see train_step)
        self.fused_optimizer_apply = bool(fused_optimizer_apply)
        self.query_features = query_features
        self.candidate_features = candidate_features
        if candidate_id_col not in [f.name for f in candidate_features]:
            raise ValueError(f"candidate_id_col {candidate_id_col} not a candidate feature")
        if any(f.name == candidate_id_col and f.is_sequence for f in candidate_features):
            raise ValueError(f"candidate_id_col {candidate_id_col} may not be a sequence feature")
        self.candidate_id_col = candidate_id_col
        self.device = device if device is not None else default_device()
        gen = make_generator(seed)
        # the temperature folds into the query side's normalisation scale:
        # logits = (q / |q| / T) . (c / |c|), so no loss or index kernel changes
        self.query_tower = Tower(query_features, joint_embedding_size, query_tower_units, self.device, gen,
                                 normalize=self.normalize_embeddings,
                                 output_scale=1.0 / temperature if temperature is not None else 1.0)
        self.candidate_tower = Tower(candidate_features, joint_embedding_size, candidate_tower_units, self.device, gen,
                                     normalize=self.normalize_embeddings)
        self.logq_correction = LogQCorrection(candidate_prob_lookup) if candidate_prob_lookup else None
        self._logq_rows: Optional[torch.Tensor] = None
        self.optimizer = None
        self.last_step: Optional[TrainStep] = None  # the last train_step's state, for inspection
        self.loss = InBatchSoftmaxCrossEntropy()
        self.initialise_model()

    @property
    def towers(self) -> List[Tower]:
        return [self.query_tower, self.candidate_tower]

    # ------------------------------------------------------------------
    def _split(self, x: Dict[str, Any]):
        q = {f.name: x[f.name] for f in self.query_features}
        c = {f.name: x[f.name] for f in self.candidate_features}
        return q, c

    def call(self, x: Dict[str, Any], training: bool = True) -> torch.Tensor:
        """[Q, C] scores of every query against every candidate of the batch
        (two_tower_model.py:65-92); materialised.  An INSPECTION path, not
        the hot path: fit / train_step / the graphed and sharded steps never
        call it (they never form [B, B]: losses.towers_inbatch_softmax_xent,
        the fused tt_inbatch kernels).  The score matrix is libtt's
        (hip_ops.score_matrix, bf16x3 MFMA: fp32-faithful); with gradients
        enabled it is hip_ops.ScoreMatrix, whose backward GEMMs (dQ = G.C,
        dC = G^T.Q) run on the same kernel, so a caller can differentiate
        through it (the reference's tf.matmul semantics)."""
        q, c = self._split(x)
        with torch.set_grad_enabled(training and torch.is_grad_enabled()):
            qe, ce = self.query_tower.call(q), self.candidate_tower.call(c)
            if torch.is_grad_enabled():
                return hip_ops.ScoreMatrix.apply(qe, ce)
            return hip_ops.score_matrix(qe, ce)

    def candidate_logq(self, x: Dict[str, Any]) -> Optional[torch.Tensor]:
        """Per-example log p(candidate) [B] for the logQ correction, or None."""
        if self.logq_correction is None:
            return None
        if LOGQ_KEY in x:
            v = x[LOGQ_KEY]
            v = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, np.float32))
            return v.reshape(-1).to(device=self.device, dtype=torch.float32).contiguous()
        if self._logq_rows is None:
            feat = next(f for f in self.candidate_features if f.name == self.candidate_id_col)
            self._logq_rows = self.logq_correction.row_table(feat, self.device)
        ids = x[self.candidate_id_col]
        ids = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(np.asarray(ids))
        ids = ids.reshape(-1).to(self.device, torch.int32).contiguous()
        # one libtt gather launch: the logq table is a 1-wide embedding of the
        # candidate ids (ids outside the table read 0 = the missing-id value)
        out = torch.empty(ids.numel(), 1, dtype=torch.float32, device=self.device)
        hip_ops.gather_grouped([(self._logq_rows.view(-1, 1), ids, 0)], ids.numel(), out)
        return out.view(-1)

    def candidate_ids(self, x: Dict[str, Any]) -> Optional[torch.Tensor]:
        """The batch's encoded candidate ids [B] (int32) for the loss when
        remove_accidental_hits is set, else None.  A view of the batch's
        column when that is an int32 device tensor already (the graphed
        step's static word buffer): no copy, nothing to re-capture."""
        if not self.remove_accidental_hits:
            return None
        ids = x[self.candidate_id_col]
        ids = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(np.asarray(ids))
        return ids.reshape(-1).to(self.device, torch.int32).contiguous()

    def sample_weights(self, x: Dict[str, Any]) -> Optional[torch.Tensor]:
        """The batch's normalised sample weights [B] (fp32, on the device), or
        None for a batch without WEIGHT_KEY.  A view of the batch's column
        when that is an fp32 device tensor already (the graphed step's static
        word buffer): no copy, nothing to re-capture."""
        if WEIGHT_KEY not in x:
            return None
        v = x[WEIGHT_KEY]
        v = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, np.float32))
        return v.reshape(-1).to(device=self.device, dtype=torch.float32).contiguous()

    def _logq_call(self, x: Dict[str, Any]):
        """(segments, out) of the logQ lookup as a 1-wide gather call, or None
        when logQ comes another way (precomputed in the batch / disabled)."""
        if self.logq_correction is None or LOGQ_KEY in x:
            return None
        ids = x[self.candidate_id_col]
        if not isinstance(ids, torch.Tensor) or ids.device.type != "cuda" or ids.dtype != torch.int32:
            return None
        if self._logq_rows is None:
            feat = next(f for f in self.candidate_features if f.name == self.candidate_id_col)
            self._logq_rows = self.logq_correction.row_table(feat, self.device)
        ids = ids.reshape(-1).contiguous()
        out = torch.empty(ids.numel(), 1, dtype=torch.float32, device=self.device)
        return [(self._logq_rows.view(-1, 1), ids, 0)], out

    # ------------------------------------------------------------------ mixed negative sampling
    def set_candidate_catalogue(self, catalogue) -> None:
        """Attach the pkg.modelling.dataset.CandidateCatalogue the M extra
        negatives of a training step are drawn from (num_sampled_negatives).
        It must hold the candidate tower's features; it is not saved with the
        model.  Attaching one restarts the sampler at step 0."""
        from pkg.modelling.dataset import CandidateCatalogue

        if catalogue is not None:
            if not isinstance(catalogue, CandidateCatalogue):
                raise TypeError("set_candidate_catalogue takes a pkg.modelling.dataset.CandidateCatalogue")
            seq = [f.name for f in self.candidate_features if f.is_sequence]
            if seq:
                raise NotImplementedError(f"mixed negative sampling does not support sequence features in the "
                                          f"candidate tower (feature {seq[0]!r})")
            want = list(dict.fromkeys(f.name for f in self.candidate_features))
            if catalogue.feature_names != want:
                raise ValueError(f"the catalogue holds {catalogue.feature_names}, the candidate tower takes {want}")
            if catalogue.words.device != self.device:
                raise ValueError(f"the catalogue lives on {catalogue.words.device}, the model on {self.device}")
        self.candidate_catalogue = catalogue
        self._mixed_buffers, self._mixed_logq = {}, {}
        self._mixed_step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._mixed_status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._device_fit_graph = None  # a cached fit graph holds the old catalogue's addresses

    def _warn_mixed_hits(self) -> None:
        if self.num_sampled_negatives is not None and not self.remove_accidental_hits and not self._mixed_warned:
            self._mixed_warned = True
            logger.warning("num_sampled_negatives is set without remove_accidental_hits: a sampled candidate equal to "
                           "a row's own positive is scored as a negative of that row")

    def mixture_logq_table(self, batch_size: int) -> torch.Tensor:
        """The mixture's logQ per embedding row r of the candidate-id feature
        at this batch size: log((B p_r + M / N) / (B + M)), p_r the lookup's
        (fp32) probability of vocab[r - 1], 1 for rows outside the lookup (the
        reference's rule, the OOV row 0 included), N the catalogue size.
        Built on the host in fp64, rounded to fp32, cached per (B, M)."""
        B, M, N = int(batch_size), self.num_sampled_negatives, self.candidate_catalogue.num_rows
        key = (B, M)
        if key not in self._mixed_logq:
            feat = next(f for f in self.candidate_features if f.name == self.candidate_id_col)
            keys = list(self.logq_correction.lookup.keys())
            rows = feat.encode(np.asarray(keys, dtype=str)) if keys else np.zeros(0, np.int64)
            if np.any(rows == 0):
                missing = [k for k, r in zip(keys, rows.tolist()) if r == 0][:3]
                raise ValueError(f"candidate_prob_lookup has ids outside the {feat.name} vocab (e.g. {missing}); "
                                 "mixed negative sampling reads logQ by embedding row")
            p = np.ones(len(feat.vocab) + 1, np.float64)
            p[rows] = np.asarray(list(self.logq_correction.lookup.values()), np.float32).astype(np.float64)
            table = np.log((B * p + M / N) / (B + M)).astype(np.float32)
            self._mixed_logq[key] = torch.as_tensor(table, device=self.device)
        return self._mixed_logq[key]

    def _gathered(self, step: TrainStep, pack: list, qi: torch.Tensor) -> None:
        """After a training step's gather launches: the towers' images are
        this step's where they rode along (pack), and the ids are ready."""
        for ts in step.towers:
            ts.packed = bool(pack)
        if qi.is_cuda:
            # the embedding update's id sort needs only these ids
            step.ids_ready = torch.cuda.Event()
            step.ids_ready.record()
            if step.mode == "fused":
                # fused apply (train_step): the per-tower id sorts captured
                # right after the gather (their only input), so they overlap
                # the forward instead of landing in front of the backward
                self.optimizer.prepare_towers(self.towers, ["", TOWER_C_SCOPE])

    def _gather_pack_jobs(self) -> list:
        """Both towers' MLP weight-image jobs for a training step's gather
        launch (PACK_WITH_GATHER), or none: more than 8 do not fit it, and
        each tower's forward then packs its own."""
        if not (PACK_WITH_GATHER and self.device.type == "cuda"):
            return []
        pack = [j for t in self.towers for j in t.dense.prepack_jobs(t.dense.flat.detach())]
        return pack if len(pack) <= 8 else []

    def _compute_loss_mixed(self, x: Dict[str, Any], step: TrainStep) -> torch.Tensor:
        """The training loss with num_sampled_negatives: the candidate side
        sampled and assembled by one tt_mixed_candidates launch into a
        persistent [F, B + M] buffer (so a captured step replays it), each
        tower gathered by its own launch (the logQ lookup rides with the
        candidate tower's), then the loss over B rows and B + M columns."""
        cat, M = self.candidate_catalogue, self.num_sampled_negatives
        if cat is None:
            raise RuntimeError(f"num_sampled_negatives={M} needs a candidate catalogue: call "
                               "set_candidate_catalogue(CandidateCatalogue...) before training")
        if LOGQ_KEY in x:
            raise ValueError(f"a batch carrying {LOGQ_KEY!r} cannot train with num_sampled_negatives: the sampled "
                             "columns have no such value (logQ is read by embedding row)")
        self._warn_mixed_hits()
        q, c = self._split(x)
        layer = self.candidate_tower.input_layer
        feats = {f.name: f for f in self.candidate_features}
        cols = []
        for name in cat.feature_names:
            f = feats[name]
            if f.dtype == _dtypes.string:
                cols.append(layer._ids(c[name], f))
            else:
                v = c[name] if isinstance(c[name], torch.Tensor) else torch.as_tensor(np.asarray(c[name], np.float32))
                cols.append(v.reshape(-1).to(device=self.device, dtype=torch.float32).contiguous())
        B = cols[0].numel()
        buf = self._mixed_buffers.get(B)
        if buf is None:
            buf = self._mixed_buffers[B] = torch.empty(len(cols), B + M, dtype=torch.int32, device=self.device)
        hip_ops.mixed_candidates(cols, cat.words, M, self.sampled_negatives_seed, self._mixed_step, buf,
                                 self._mixed_status)
        cm = {name: (buf[i] if feats[name].dtype == _dtypes.string else buf[i].view(torch.float32))
              for i, name in enumerate(cat.feature_names)}
        ids_all = cm[self.candidate_id_col]
        with torch.enable_grad():
            call = None
            if self.logq_correction is not None:
                out = torch.empty(B + M, 1, dtype=torch.float32, device=self.device)
                call = ([(self.mixture_logq_table(B).view(-1, 1), ids_all, 0)], out)
            pack = self._gather_pack_jobs()
            (qi,) = InputLayer.gather_many([self.query_tower.input_layer], [q], pack_jobs=pack or None)
            (ci,) = InputLayer.gather_many([layer], [cm], extra=[call] if call is not None else ())
            self._gathered(step, pack, qi)
            logq = call[1].view(-1) if call is not None else None
            return self.tower_loss(qi, ci, logq, ids_all if self.remove_accidental_hits else None,
                                   self.sample_weights(x), step=step)

    def compute_loss(self, x: Dict[str, Any], training: bool = True, *, step: Optional[TrainStep] = None
                     ) -> torch.Tensor:
        """The batch's loss.  step: train_step's TrainStep; a training loss
        without one is a plain step's (nothing applied inside its backward)."""
        if training and step is None:
            step = TrainStep()
        if training and self.num_sampled_negatives is not None:
            return self._compute_loss_mixed(x, step)
        q, c = self._split(x)
        with torch.set_grad_enabled(training):
            call = self._logq_call(x)  # rides in the towers' gather launch
            # ... and so do the towers' MLP weight images of this forward (at most 8 jobs)
            pack = self._gather_pack_jobs() if training else []
            qi, ci = InputLayer.gather_many([self.query_tower.input_layer, self.candidate_tower.input_layer], [q, c],
                                            extra=[call] if call is not None else (), pack_jobs=pack or None)
            if training:
                self._gathered(step, pack, qi)
            logq = call[1].view(-1) if call is not None else self.candidate_logq(x)
            return self.tower_loss(qi, ci, logq, self.candidate_ids(x), self.sample_weights(x), step=step)

    def tower_loss(self, qi: torch.Tensor, ci: torch.Tensor, logq: Optional[torch.Tensor],
                   ids: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None, *,
                   step: Optional[TrainStep] = None) -> torch.Tensor:
        """Loss from the gathered tower inputs: with gradients, both MLPs and the
        in-batch loss run as one autograd node (losses.towers_inbatch_softmax_xent).
        ids: candidate_ids(x) (accidental hits removed), or None.  weights:
        sample_weights(x), or None (an unweighted batch: the calls as ever).
        step: the TrainStep this loss belongs to (compute_loss), or None."""
        wkw = {} if weights is None else {"weights": weights, "weight_scale": float(self.sample_weight_scale)}
        if self.num_hard_negatives is not None:  # hard-negative mining, on every path through here
            wkw["num_hard_negatives"] = self.num_hard_negatives
        if torch.is_grad_enabled():
            return towers_inbatch_softmax_xent(qi, ci, self.query_tower.dense, self.candidate_tower.dense, logq,
                                               self.loss.reduction, ids=ids, step=step, **wkw)
        sq, sc = self.query_tower.dense, self.candidate_tower.dense
        if sq.normalize or sc.normalize:  # both outputs normalised in one launch, after both towers
            q, c, _ = normalized_outputs(sq, sc, sq.forward_acts(qi, sq.flat.detach())[-1],
                                         sc.forward_acts(ci, sc.flat.detach())[-1])
            return self.loss(q, c, logq, ids, **wkw)
        return self.loss(sq(qi), sc(ci), logq, ids, **wkw)

    def compile(self, loss=None, optimizer=None, **kwargs) -> None:
        """Keras-style compile: the loss must be the in-batch softmax CE
        (CategoricalCrossentropy(from_logits=True, reduction=SUM) in the
        reference, runner.py:78-83)."""
        if loss is not None:
            if not isinstance(loss, InBatchSoftmaxCrossEntropy):
                raise TypeError("loss must be pkg.modelling.losses.CategoricalCrossentropy(from_logits=True, ...)")
            self.loss = loss
        if optimizer is not None:
            self._check_clipping(optimizer)
            self.optimizer = optimizer
            # a cached fit graph holds the old optimizer's slot addresses
            self._device_fit_graph = None
        self._warn_mixed_hits()

    def _check_clipping(self, optimizer) -> None:
        if self.fused_optimizer_apply and getattr(optimizer, "clips", False):
            raise ValueError("fused_optimizer_apply applies each tower's update inside the backward; gradient "
                             "clipping (clipvalue / clipnorm / global_clipnorm) needs every gradient before any "
                             "update: use one or the other")

    def check_optimizer_status(self) -> None:
        """Raise if a sparse apply since the last check refused stale or
        foreign keys (tt_sparse_status; one stream sync)."""
        check = getattr(self.optimizer, "check_status", None)
        if check is not None and self.device.type == "cuda":
            check(self.device)

    def train_step(self, data: Dict[str, Any]) -> Dict[str, torch.Tensor]:
        """One optimisation step on a batch of positive pairs; returns the
        (device) loss without synchronising.  With fused_optimizer_apply (opt-in,
        Adagrad on the GPU) each tower's dense and sparse updates are applied
        inside the backward, the moment that tower's gradients exist (the
        candidate tower's beside the query tower's backward); the updates are
        the same as applying them afterwards (each table and MLP buffer is
        touched by one tower only; tests/test_model_gpu.py checks bit-identity)."""
        from pkg.modelling.optimizer_factory import Adagrad

        if self.optimizer is None:
            raise RuntimeError("call compile(optimizer=...) before training")
        # a clipping optimizer needs every gradient before any update: no
        # update from inside the backward, apply_gradients after it
        clips = bool(getattr(self.optimizer, "clips", False))
        self._check_clipping(self.optimizer)
        fused = self.fused_optimizer_apply and isinstance(self.optimizer, Adagrad) and self.device.type == "cuda"
        dense_early = (not fused and not clips and DENSE_EARLY and isinstance(self.optimizer, Adagrad)
                       and self.device.type == "cuda")
        step = self.last_step = TrainStep("fused" if fused else "dense_early" if dense_early else "plain")
        for t, ts in zip(self.towers, step.towers):
            ts.separate_launches = bool(fused)
            if dense_early and FUSED_DENSE_WGRAD:
                opt = self.optimizer
                (acc,) = opt._slot(t.dense.flat, 1, opt.initial_accumulator_value)
                ts.adagrad = (acc, opt.learning_rate, opt.epsilon)
        if fused:
            step.on_tower = functools.partial(self._apply_tower, step)
            # each tower's embedding update the moment its input gradient
            # exists (the weight gradients follow it on that tower's stream)
            step.on_dx = functools.partial(self._apply_tower_sparse, step) if _tower_mod.IGRAD_FIRST else None
        elif dense_early:
            step.on_tower = functools.partial(self._apply_dense_tower, step)
        loss = self.compute_loss(data, training=True, step=step)  # fused: issues the per-tower id sorts
        fwd_done = None
        if not fused and hasattr(self.optimizer, "prepare") and loss.is_cuda:
            # the id sort waits for the gather only (compute_loss recorded the
            # event), not the whole forward: 6.6 us/step on the C3 step over 6
            # interleaved pairs
            fwd_done = step.ids_ready
        for t in self.towers:
            t.dense.flat.grad = None
        if getattr(self, "_one", None) is None or self._one.device != loss.device:
            self._one = torch.ones((), dtype=loss.dtype, device=loss.device)
        loss.backward(self._one)  # a persistent seed: no ones-fill launch per step
        step.on_tower = step.on_dx = None  # what stays as last_step is plain data, with no way back to the model
        if fused:
            self.optimizer.iterations += 1
            # the update is applied: a later apply_gradients must not apply it again
            for t in self.towers:
                t.dense.flat.grad = None
                t.input_layer.last_grad = None
        else:
            for i in step.dense_done:  # applied inside the backward: not again
                self.towers[i].dense.flat.grad = None
            if fwd_done is not None:
                # the embedding update's id sort needs only the forward's ids; issued
                # after the backward (so the backward's chains are launched first)
                # but ordered only after the forward, it overlaps the backward
                self.optimizer.prepare(self.towers, after=fwd_done)
            self.optimizer.apply_gradients(self.towers)
        return {"loss": loss.detach()}

    # the step's callbacks (train_step binds the TrainStep: on_tower(i, ...), on_dx(i, dx))
    def _apply_tower(self, step: TrainStep, i: int, input_grad: Optional[torch.Tensor],
                     flat_grad: torch.Tensor) -> None:
        if i in step.sparse_done:  # its embedding update ran at the input gradient
            self.optimizer.apply_dense(self.towers[i], flat_grad)
            return
        self.optimizer.apply_tower(self.towers[i], input_grad, flat_grad)

    def _apply_tower_sparse(self, step: TrainStep, i: int, input_grad: Optional[torch.Tensor]) -> None:
        self.optimizer.apply_tower_sparse(self.towers[i], input_grad)
        step.sparse_done.add(i)

    def _apply_dense_tower(self, step: TrainStep, i: int, input_grad: Optional[torch.Tensor],
                           flat_grad: torch.Tensor) -> None:
        st, applied = self.towers[i].dense, step.towers[i].fused_layers
        if applied:  # the weight-gradient launches applied those layers' step
            for li, (w_off, fi, fo, _) in enumerate(st.layout):
                if li not in applied:  # a layer outside tt_mlp_wgrad's contract
                    n = (fi + 1) * fo
                    (acc,) = self.optimizer._slot(st.flat, 1, self.optimizer.initial_accumulator_value)
                    hip_ops.dense_adagrad(st.flat.data[w_off:w_off + n], acc[w_off:w_off + n],
                                          flat_grad[w_off:w_off + n], self.optimizer.learning_rate,
                                          self.optimizer.epsilon)
        else:
            self.optimizer.apply_dense(self.towers[i], flat_grad)
        step.dense_done.add(i)

    def fit(self, dataset: Iterable[Dict[str, Any]], epochs: int = 1, callbacks=None,
            use_graph: bool = False) -> Dict[str, List[float]]:
        """Train for `epochs` passes; returns {"loss": [mean batch loss per epoch]}
        (Keras' loss metric is the running mean over the epoch's batches)."""
        from pkg.modelling.dataset import DeviceDataset

        if getattr(dataset, "weight_scale", None) is not None:  # w_max of the dataset's "__weight__" column
            self.sample_weight_scale = float(dataset.weight_scale)
        if use_graph and isinstance(dataset, DeviceDataset) and dataset.fn is None and dataset.batch_size:
            return self._fit_device(dataset, epochs, callbacks)
        history: Dict[str, List[float]] = {"loss": []}
        graphed: Optional[GraphedTrainStep] = None
        for epoch in range(epochs):
            total = torch.zeros((), dtype=torch.float64, device=self.device)
            n = 0
            for batch in dataset:
                bs = next(iter(batch.values())).shape[0]
                if use_graph and graphed is None:
                    # the single warm-up step IS this batch's optimisation step
                    graphed = GraphedTrainStep(self, batch, warmup=1)
                    out = graphed.warmup_out
                elif use_graph and bs == graphed.batch_size:
                    out = graphed(batch)
                else:  # eager (also the partial last batch of a graphed epoch)
                    out = self.train_step(batch)
                total += out["loss"].double()
                n += 1
            self.check_optimizer_status()
            mean = float(total.item()) / max(n, 1)
            history["loss"].append(mean)
            logger.info(f"epoch {epoch + 1}/{epochs}: loss {mean:.6f} over {n} batches")
            for cb in callbacks or []:
                if callable(cb):
                    cb(epoch, {"loss": mean})
        return history

    def _fit_device(self, ds, epochs: int, callbacks) -> Dict[str, List[float]]:
        """fit over an HBM-resident DeviceDataset: each full batch is one replay
        of a graph that takes the batch on the device and trains on it; the
        partial last batch runs eagerly.  One host sync per epoch (the loss)."""
        history: Dict[str, List[float]] = {"loss": []}
        B, nfull = int(ds.batch_size), ds.full_batches
        rem = ds.num_rows - nfull * B
        graphed = None
        for epoch in range(epochs):
            ds.begin_epoch()
            todo = nfull
            # before every epoch's replays (the eager partial batch of the last
            # one, or other work since, may have regrown a workspace)
            graphed = getattr(self, "_device_fit_graph", None)
            if graphed is not None and not graphed.reusable(self, ds):
                graphed = self._device_fit_graph = None
            if todo and graphed is None:
                graphed = GraphedTrainStep(self, None, warmup=1, source=ds)  # warm-up = this epoch's batch 0
                self._device_fit_graph = graphed
                todo -= 1
            elif graphed is not None:
                graphed.loss_total.zero_()
            for _ in range(todo):
                graphed.graph.replay()
            total = graphed.loss_total.clone() if graphed is not None else torch.zeros(
                (), dtype=torch.float64, device=self.device)
            if rem:
                total += self.train_step(ds.view(ds.take(rem)))["loss"].double()
            ds.check_status()
            self.check_optimizer_status()
            n = nfull + (1 if rem else 0)
            mean = float(total.item()) / max(n, 1)
            history["loss"].append(mean)
            logger.info(f"epoch {epoch + 1}/{epochs}: loss {mean:.6f} over {n} batches (device-resident, graphed)")
            for cb in callbacks or []:
                if callable(cb):
                    cb(epoch, {"loss": mean})
        return history

    @classmethod
    def create_from_schema(cls, schema: Schema, candidate_id_col: str, **kwargs) -> "TwoTowerModel":
        """Instance from a Schema (two_tower_model.py:132-158)."""
        return TwoTowerModel(
            query_features=schema.query_features,
            candidate_features=schema.candidate_features,
            candidate_id_col=candidate_id_col,
            joint_embedding_size=schema.model_config.joint_embedding_size,
            query_tower_units=schema.model_config.query_tower_units,
            candidate_tower_units=schema.model_config.candidate_tower_units,
            candidate_prob_lookup=schema.training_config.candidate_prob_lookup,
            **kwargs,
        )

    def get_input_signature(self) -> Dict[str, TensorSpec]:
        return {f.name: TensorSpec((None, f.sequence_length if f.is_sequence else 1), f.dtype, f.name)
                for f in self.candidate_features + self.query_features}

    def state_dict(self) -> Dict[str, torch.Tensor]:
        sd = {f"query_tower.{k}": v for k, v in self.query_tower.state_dict().items()}
        sd.update({f"candidate_tower.{k}": v for k, v in self.candidate_tower.state_dict().items()})
        return sd

    def save(self, model_path: str) -> None:
        """Save the two-tower model and each tower separately in the
        two_tower / query_tower / candidate_tower entries of the model
        directory (two_tower_model.py:176-205): weights (.pt, weights-only),
        architecture (.json) and vocabularies (.npz) — pkg.modelling.export."""
        from pkg.modelling import export

        base = os.path.dirname(model_path)
        os.makedirs(base or ".", exist_ok=True)
        logging.info(f"Saving two_tower, query_tower, candidate_tower under {base or '.'}")
        export.save_two_tower(self, os.path.join(base, "two_tower"))
        export.save_tower(self.query_tower, os.path.join(base, "query_tower"))
        export.save_tower(self.candidate_tower, os.path.join(base, "candidate_tower"))

    @classmethod
    def load(cls, model_path: str, device: Optional[torch.device] = None) -> "TwoTowerModel":
        """The model saved by save(model_path) (compile() it again to train)."""
        from pkg.modelling import export

        return export.load_two_tower(os.path.join(os.path.dirname(model_path), "two_tower"), device)


class GraphedTrainStep:
    """Capture TwoTowerModel.train_step once as a hipGraph and replay it.

    The batch lives in two static device buffers (int32 ids [K, B], float32
    values [F, B]; a sequence feature's [B, L] ids take L consecutive int rows
    and are read through the transposed view of those rows, so no copy is made
    inside the graph); a replay is one D2D copy per buffer (or none, for
    `replay()`), then the whole step — gathers, MLP GEMMs, the fused
    loss kernels and the optimizer kernels — with no Python or launch
    overhead.  Warm-up steps (run eagerly on a side stream before capture)
    are real optimisation steps on the example batch.  Requires an optimizer
    whose kernels do not depend on the host step count: Adagrad, or Adam with
    its step count moved to the device (Adam.enable_device_clock, called here
    before the warm-up: the captured step starts with one launch that advances
    the device's count and takes that step's two coefficients from a
    host-filled table, so every replay is the next Adam step and
    `optimizer.iterations` reports the device's count)."""

    def __init__(self, model: TwoTowerModel, example_batch: Optional[Dict[str, Any]], warmup: int = 2,
                 source=None):
        """source: a pkg.modelling.dataset.DeviceDataset whose next batch is
        taken on the device inside the graph (tt_batch_take, cursor in device
        memory) — every replay then trains on the dataset's next batch and
        adds its loss to `loss_total` (fp64, device) with no host work."""
        from pkg.modelling.optimizer_factory import Adagrad, Adam

        if isinstance(model.optimizer, Adam):
            # before the warm-up steps: they and the capture then take the same
            # launches (ValueError for betas without a coefficient table)
            model.optimizer.enable_device_clock(model.device)
        elif not isinstance(model.optimizer, Adagrad):
            raise ValueError("graph capture needs the Adagrad or the Adam optimizer "
                             f"(got {type(model.optimizer).__name__})")
        self.model = model
        self.source = source
        if source is not None:
            if not source.batch_size:
                raise ValueError("a graphed DeviceDataset source needs a batch_size")
            self.int_keys, self.float_keys = list(source.int_keys), list(source.float_keys)
            self.int_widths = dict(source.int_widths)
            self.batch_size = int(source.batch_size)
            ex = None
        else:
            ex = {k: self._flat(self._to_dev(v, model.device)) for k, v in example_batch.items()}
            self.int_keys = sorted(k for k, v in ex.items() if v.dtype != torch.float32)
            self.float_keys = sorted(k for k, v in ex.items() if v.dtype == torch.float32)
            # word rows per int key: L for a [B, L] column, none recorded for [B]
            self.int_widths = {k: ex[k].shape[1] for k in self.int_keys if ex[k].dim() == 2}
            self.batch_size = next(iter(ex.values())).shape[0]
        B = self.batch_size
        K, F = len(self.int_keys) + sum(w - 1 for w in self.int_widths.values()), len(self.float_keys)
        # one [K + F, B] buffer of 32-bit words: int rows first, then float rows
        # (the DeviceDataset layout, so one take launch fills the whole batch)
        self._wbuf = torch.empty(max(K + F, 1), B, dtype=torch.int32, device=model.device)
        self._ibuf = self._wbuf[:K] if K else torch.empty(1, B, dtype=torch.int32, device=model.device)
        self._fbuf = (self._wbuf[K:K + F].view(torch.float32) if F
                      else torch.empty(1, B, dtype=torch.float32, device=model.device))
        self.static, row = {}, 0
        for k in self.int_keys:
            w = self.int_widths.get(k)
            self.static[k] = self._ibuf[row] if w is None else self._ibuf[row:row + w].t()
            row += w or 1
        self.static.update({k: self._fbuf[i] for i, k in enumerate(self.float_keys)})
        self.loss_total = torch.zeros((), dtype=torch.float64, device=model.device)
        if ex is not None:
            self.load(ex)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(warmup, 1)):
                out = self._step()
            self.warmup_out = {k: v.clone() for k, v in out.items()}
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: other host threads (a process group's watchdog, the
        # dataset's order prefetch) may query events while this thread captures
        self._graph_events: list = []  # events created during the capture live as long as the graph
        with hip_ops.capture_guard(self._graph_events), torch.cuda.graph(self.graph,
                                                                          capture_error_mode="thread_local"):
            self.out = self._step()
        # what the captured pointers refer to (see reusable)
        self.optimizer = model.optimizer
        # a weighted step (rows, fold, cols, tt_sum) with w_max a constant of the graph
        self.weight_scale = float(model.sample_weight_scale) if WEIGHT_KEY in self.static else None
        # mixed negative sampling: M and the catalogue whose words the captured sampler reads
        self.mixed = (model.num_sampled_negatives, model.candidate_catalogue)
        self.ws_snapshot = hip_ops.Workspace.snapshot(owner=self.graph)

    def reusable(self, model: "TwoTowerModel", source=None, batch: Optional[Dict[str, Any]] = None) -> bool:
        """True while a replay still trains `model` from `source` through the
        buffers it was captured with: same optimizer object (its slots), no
        libtt workspace regrown or cleared since the capture.  Sample weights:
        a graph captured without "__weight__" is refused for a source (or
        `batch`) that carries it and the other way round, and so is one
        captured with another sample_weight_scale."""
        keys = source.float_keys if source is not None else batch
        weighted = self.weight_scale is not None
        if keys is not None and (WEIGHT_KEY in keys) != weighted:
            return False
        if weighted and self.weight_scale != float(model.sample_weight_scale):
            return False
        if self.mixed[0] != model.num_sampled_negatives or self.mixed[1] is not model.candidate_catalogue:
            return False  # captured with another M or catalogue
        return (self.model is model and self.source is source and self.optimizer is model.optimizer
                and (source is None or int(source.batch_size) == self.batch_size)
                and hip_ops.Workspace.unchanged(self.ws_snapshot))

    def _step(self) -> Dict[str, torch.Tensor]:
        if self.source is not None:
            self.source.take(self.batch_size, out=self._wbuf)
        out = self.model.train_step(self.static)
        if self.source is not None:
            self.loss_total += out["loss"].double()
        return out

    @staticmethod
    def _to_dev(v, device):
        t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
        return t.to(device)

    @staticmethod
    def _flat(t: torch.Tensor) -> torch.Tensor:
        """[B] for a one-value column ([B] or [B, 1]); an int [B, L > 1] column keeps its axis."""
        if t.dim() == 2 and t.shape[1] > 1 and t.dtype != torch.float32:
            return t
        return t.reshape(-1)

    def _int_rows(self, k: str, t: torch.Tensor) -> torch.Tensor:
        """Key k's batch as its [rows, B] block of the int buffer."""
        w = self.int_widths.get(k)
        t = t.to(torch.int32)
        return t.reshape(1, -1) if w is None else t.reshape(-1, w).t()

    def pack(self, batch: Dict[str, Any]):
        """Device buffers laid out like the static batch (copy with one D2D each)."""
        self._check_keys(batch)
        ib = torch.cat([self._int_rows(k, self._to_dev(batch[k], self.model.device))
                        for k in self.int_keys]) if self.int_keys else self._ibuf.clone()
        fb = torch.stack([self._to_dev(batch[k], self.model.device).reshape(-1).to(torch.float32)
                          for k in self.float_keys]) if self.float_keys else self._fbuf.clone()
        return ib.contiguous(), fb.contiguous()

    def _check_keys(self, batch: Dict[str, Any]) -> None:
        """A step captured with sample weights takes weighted batches only, one
        captured without them unweighted ones only (the graph holds one or the
        other chain of launches)."""
        if (WEIGHT_KEY in batch) != (WEIGHT_KEY in self.static):
            raise ValueError(f"this step was captured {'with' if WEIGHT_KEY in self.static else 'without'} "
                             f"{WEIGHT_KEY}; the batch comes {'with' if WEIGHT_KEY in batch else 'without'} it "
                             "(capture another GraphedTrainStep)")

    def load(self, batch: Dict[str, Any]) -> None:
        self._check_keys(batch)
        for k, v in batch.items():
            self.static[k].copy_(self._to_dev(v, self.model.device).reshape(self.static[k].shape), non_blocking=True)

    def replay(self) -> Dict[str, torch.Tensor]:
        self.graph.replay()
        return self.out

    def __call__(self, batch: Optional[Dict[str, Any]] = None, packed=None) -> Dict[str, torch.Tensor]:
        if packed is not None:
            self._ibuf.copy_(packed[0], non_blocking=True)
            if self.float_keys:
                self._fbuf.copy_(packed[1], non_blocking=True)
        elif batch is not None:
            self.load(batch)
        return self.replay()
