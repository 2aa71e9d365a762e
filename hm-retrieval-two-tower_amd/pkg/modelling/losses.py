"""In-batch softmax cross-entropy with eye labels, fused on the GPU.

Replaces, in one autograd node, the reference's chain
  TwoTowerModel.call matmul          (two_tower_model.py:92)
  LogQCorrection                     (two_tower_model.py:113-116)
  labels = eye(B); CategoricalCrossentropy(from_logits=True, reduction=SUM)
                                     (two_tower_model.py:119-122, runner.py:78-83)
The forward runs both libtt passes (rows: lse, row loss, dQ; cols: dC) and
keeps dQ, dC for the backward, which only scales them by the incoming
gradient.  The [B, B] score matrix never exists.
"""
from __future__ import annotations

import contextlib
import functools
import os
import types

from typing import Optional

import torch

from pkg.modelling import hip_ops
from pkg.modelling.models.tower import backward_acts_pair, forward_acts_pair, pair_compatible

__all__ = ["InBatchSoftmaxCrossEntropy", "inbatch_softmax_xent", "towers_inbatch_softmax_xent",
           "global_inbatch_grads", "global_towers_inbatch_softmax_xent", "weighted_inbatch_grads", "TOWER_C_SCOPE"]


def x3_scores() -> bool:
    """TT_INBATCH_X3=1 (read at each call): the in-batch loss with
    fp32-faithful products (S and P.V as bf16x3 products) on every path: the
    single-device step (hip_ops.inbatch_fused(x3=True)), the global-negatives
    data-parallel step (global_inbatch_grads: the fused entry at one rank,
    hip_ops.inbatch_rows / inbatch_cols(x3=True) on every rank otherwise) and
    the no-grad evaluation loss (inbatch_softmax_xent).  Accuracy at trained
    score magnitudes (|S| ~ 100), where the default bf16 operands drift to
    ~8e-3: asserted 1e-3 in dQ/dC and 1e-4 in loss against fp64, measured
    <= 8.5e-6.  2.0-2.4x the default loss's time.  A captured
    step keeps the mode it was captured with: the flag is read when the step
    runs eagerly, not when its graph replays.  The default is the
    bf16-operand contract (include/tt.h K5-K7)."""
    return os.environ.get("TT_INBATCH_X3", "0") == "1"


# ids (every loss below, optional): the int32 candidate id of each row's
# positive.  Given, accidental hits are removed: a column j other than row i's
# own with ids[j] == ids[i] (the same article again in the batch) is no
# negative of row i, in the loss and in both gradients (include/tt.h,
# tt_inbatch_*_hits; TensorFlow Recommenders' remove_accidental_hits).  Ids
# are compared for equality only, so all out-of-vocabulary rows (id 0) count
# as one candidate.  The reference has no such option: ids=None is its loss.


# weights (every loss below, optional): per-example sample weights, an fp32
# [B] device tensor of NORMALISED weights w_i / w_max in [0, 1], with
# weight_scale = w_max (TensorFlow Recommenders' Retrieval task sample_weight,
# Keras fit(sample_weight=...)): the loss is sum_i w_max w_i l_i, "mean"
# divides by B (Keras' rule).  The pass kernels do not change: the rows pass
# runs as it is, hip_ops.inbatch_weight_rows folds w into the lse and row_loss
# the cols pass reads and scales dq in place (one launch), the cols pass
# returns the weighted dc, and w_max goes into the loss scale and the
# backward's scalar (include/tt.h, tt_inbatch_weight_rows).  A weight outside
# [0, 1] turns the loss NaN.  weights=None issues the calls it always issued.


# num_hard_negatives (every loss below, optional): hard-negative mining, a
# positive int K (TensorFlow Recommenders' Retrieval(num_hard_negatives=K)).
# Of each row's negatives only the K with the largest logits S' = q_i . c_j -
# logq[j] keep their weight in the loss and in both gradients; it applies
# after temperature / cosine scoring, logQ and accidental hits, as in TFRS.
# A selection kernel finds each row's threshold thr[i], the midpoint of its
# K-th and (K+1)-th largest negative score, and the HARD form of the pass
# kernels drops every negative below it (include/tt.h, tt_inbatch_*_hard).
# Negatives that tie the K-th value are all kept — the one departure from
# tf.math.top_k's index tie-break.  K at or above the number of negatives is
# the loss without mining, bit for bit.  None issues the calls it always
# issued.


# Extra negatives (the single-device losses below): c may have more rows than
# q.  Rows past len(q) are negatives of every row and positives of none — the
# candidates mixed negative sampling draws from the whole catalogue
# (TwoTowerModel(num_sampled_negatives=M)); logq and ids then have len(c)
# entries, ids[i] being row i's id as well.  The rows pass and the selection
# take the wider c as they are, the cols pass is its MIXED form (include/tt.h,
# "mixed negatives").  c with len(q) rows issues the calls it always issued.


def _row_ids(ids, q, c):
    """The rows' ids of a loss whose ids cover every column: with extra
    negatives the first len(q), otherwise ids as it is."""
    return ids if ids is None or c.shape[0] == q.shape[0] else ids[:q.shape[0]]


def _check_hard(k):
    if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k < 1):
        raise ValueError(f"num_hard_negatives must be a positive int or None, got {k!r}")
    return k


def weighted_inbatch_grads(q, c, logq, weights, ids=None, x3: Optional[bool] = None,
                           num_hard_negatives: Optional[int] = None):
    """(wloss [B], dq, dc) of the weighted single-device loss: rows, fold,
    cols, with the operands and ids the unweighted entries take;
    num_hard_negatives: select, rows, fold, cols."""
    hard = _check_hard(num_hard_negatives)
    kw = {"x3": x3_scores() if x3 is None else x3, "row_ids": _row_ids(ids, q, c), "col_ids": ids}
    if hard is not None:
        kw["thr"] = hip_ops.inbatch_hard_threshold(q, c, logq, hard, **kw)
    lse, row_loss, dq = hip_ops.inbatch_rows(q, c, logq, **kw)
    lse_w, row_loss_w, wloss = hip_ops.inbatch_weight_rows(weights, lse, row_loss, dq)
    if c.shape[0] != q.shape[0]:  # extra negatives: the MIXED cols pass
        kw["mixed"] = True
    dc = hip_ops.inbatch_cols(q, lse_w, c, logq, row_loss=row_loss_w, **kw)
    return wloss, dq, dc


def _fused_grads(q, c, logq, ids, hard, x3, loss_scale=None, ws=None):
    """(row_loss, dq, dc, loss) of the unweighted single-device loss through
    the fused entries, whichever they return beside these: inbatch_fused, or
    inbatch_fused_mixed where c has extra negatives (every option, its own
    preparation and workspace).  loss_scale: the loss summed by an extra
    workgroup of the entry's last launch (no tt_sum launch after it), else
    loss is None.  ws: the workspace both operands were already prepared into
    (hip_ops.inbatch_prep; the plain bf16 entry alone takes one)."""
    kw = {}
    if hard is not None:
        kw["hard_k"] = hard
    if loss_scale is not None:
        kw["loss_scale"] = loss_scale
    if c.shape[0] != q.shape[0]:
        out = hip_ops.inbatch_fused_mixed(q, c, logq, x3=x3, ids=ids, **kw)
    else:
        if ws is not None:
            kw.update(ws=ws, prepped=True)
        out = hip_ops.inbatch_fused(q, c, logq, x3=x3, ids=ids, **kw)
    return out[1], out[2], out[3], (out[-1] if loss_scale is not None else None)


class _InBatchXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, c, logq, scale, ids=None, weights=None, weight_scale=1.0, hard=None):
        if weights is not None:
            scale = scale * weight_scale
            row_loss, dq, dc = weighted_inbatch_grads(q, c, logq, weights, ids, num_hard_negatives=hard)
        else:
            row_loss, dq, dc, _ = _fused_grads(q, c, logq, ids, hard, x3_scores())
        ctx.scale = scale
        ctx.save_for_backward(dq, dc)
        return hip_ops.loss_sum(row_loss, scale)

    @staticmethod
    def backward(ctx, g):
        dq, dc = ctx.saved_tensors
        s = g * ctx.scale
        return dq * s, dc * s, None, None, None, None, None, None


_SIDE: dict = {}

# Workspace scope of the candidate tower's work on its own stream (the fused
# train step sorts and applies that tower's embedding update in this scope).
TOWER_C_SCOPE = "tower_c"

def _tower_stream(device: torch.device) -> torch.cuda.Stream:
    """The stream the candidate tower's MLP runs on, beside the query tower's."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


# The global-negatives step runs the two towers on two streams from this many
# rows per rank (TT_GLOBAL_TOWER_STREAMS overrides; 0: always one stream).
# World-1 sharded step, interleaved pairs: 16384 rows 0.896-0.903 vs
# 0.942-0.945 ms; 2048 rows (an 8-way split) 0.579-0.605 vs 0.562-0.599.
GLOBAL_TOWER_STREAMS = int(os.environ.get("TT_GLOBAL_TOWER_STREAMS", "4096"))
# The global-negatives loss at one rank through the single-device entry
# (TT_WORLD1_FUSED=0: the rows and columns entries, as at G > 1).
WORLD1_FUSED = os.environ.get("TT_WORLD1_FUSED", "1") == "1"
# Each tower's bf16 loss operand prepared on that tower's stream
# (tt_inbatch_prep) instead of one prep of both after the join.
SPLIT_PREP = os.environ.get("TT_SPLIT_PREP", "0") == "1"
# Both towers' layers as paired launches on one stream (tower.forward_acts_pair).
TOWER_PAIR = int(os.environ.get("TT_TOWER_PAIR", "0"))


def _paired(x: torch.Tensor, stack_q, stack_c) -> bool:
    return bool(TOWER_PAIR) and x.is_cuda and pair_compatible(stack_q, stack_c)


def _hooks(step):
    """(on_tower, on_dx, (the query tower's TowerStep, the candidate tower's))
    of a train step's state (TwoTowerModel.TrainStep); of None: nothing."""
    return (None, None, (None, None)) if step is None else (step.on_tower, step.on_dx, step.towers)


def _both_towers(fork: bool, device: torch.device, tower):
    """(tower(0), tower(1)): the candidate tower's work, tower(1), issued
    first in its workspace scope and, with `fork`, on its own stream forked
    from the current one; then the query tower's, tower(0), on the current
    stream; then the join, from the fork's origin (a captured branch must not
    join a sub-branch itself)."""
    with contextlib.ExitStack() as block:
        block.enter_context(hip_ops.Workspace.scope(TOWER_C_SCOPE))
        if fork:
            side = _tower_stream(device)
            side.wait_stream(torch.cuda.current_stream())
            block.enter_context(torch.cuda.stream(side))
        cand = tower(1)
    query = tower(0)
    if fork:
        torch.cuda.current_stream().wait_stream(side)
    return query, cand


def normalized_outputs(stack_q, stack_c, q: torch.Tensor, c: torch.Tensor):
    """(q', c', invs): the two towers' joined outputs as the loss takes them.
    A stack with normalize set has its rows L2-normalised and multiplied by
    its output_scale (cosine scoring; the query side's scale is 1 /
    temperature) — ONE tt_l2norm_rows launch for both operands; invs holds
    each normalised operand's reciprocal row norms (None for one left as it
    is).  Without normalisation: (q, c, (None, None)) and no launch."""
    sides = [i for i, st in enumerate((stack_q, stack_c)) if st.normalize]
    out, invs = [q, c], [None, None]
    if sides:
        res = hip_ops.l2norm_rows([((q, c)[i], (stack_q, stack_c)[i].output_scale) for i in sides])
        for i, (y, inv) in zip(sides, res):
            out[i], invs[i] = y, inv
    return out[0], out[1], tuple(invs)


def unnormalize_grads(stack_q, stack_c, q: torch.Tensor, c: torch.Tensor, invs, dq: torch.Tensor,
                      dc: torch.Tensor) -> None:
    """dq, dc (the loss's gradients with respect to normalized_outputs' q',
    c') turned IN PLACE into the gradients with respect to the un-normalised
    q, c: ONE tt_l2norm_rows_grad launch for both.  It is linear in dq / dc,
    so the backward's device scalar applies afterwards as before."""
    jobs = [(x, inv, d, st.output_scale, d)
            for st, x, inv, d in ((stack_q, q, invs[0], dq), (stack_c, c, invs[1], dc)) if inv is not None]
    if jobs:
        hip_ops.l2norm_rows_grad(jobs)


def _two_streams(like: torch.Tensor) -> bool:
    return like.is_cuda and GLOBAL_TOWER_STREAMS > 0 and like.shape[0] >= GLOBAL_TOWER_STREAMS


class _TowersInBatchXent(torch.autograd.Function):
    """Both tower MLPs and the in-batch loss as ONE autograd node.  The two
    towers' MLPs are independent chains of small GEMMs, so the candidate
    tower's forward and backward run on a second stream concurrently with
    the query tower's (fork / join with stream waits: captured as parallel
    branches of the step's hipGraph).  The backward hands the loss's incoming
    gradient to the top layers' weight-gradient and input-gradient kernels as
    a device scalar (no separate scaling pass over dQ, dC).
    After the four tensors: logq, the stacks, the loss scale, and
      stage(q, c, ws, unnormalize) -> (loss, dq, dc): the loss stage on the
        towers' (normalised) outputs — the single-device entries or the
        global-negatives ones; it calls unnormalize(dq, dc) where it wants
        the gradients taken back to the un-normalised outputs (in place);
      fork(x) -> bool: whether the towers run on two streams;
      split_prep: each tower's bf16 loss operand prepared on its own stream
        right after its MLP, into the workspace `stage` is then given as ws;
      step: the train step's state (callbacks and per-tower TowerSteps), or None."""

    @staticmethod
    def forward(ctx, qi, ci, flat_q, flat_c, *cfg):
        logq, stack_q, stack_c, ctx.scale, stage, ctx.fork, split_prep, ctx.step = cfg
        stacks, xs, flats, tsteps = (stack_q, stack_c), (qi, ci), (flat_q, flat_c), _hooks(ctx.step)[2]
        # (extra negatives: the candidate tower runs on more rows, the towers unpaired)
        ctx.pair = _paired(qi, stack_q, stack_c) and qi.shape[0] == ci.shape[0]
        ws = None
        if ctx.pair:
            qa, ca = forward_acts_pair(stacks, xs, flats, steps=tsteps)
        else:
            if split_prep:  # (the workspace is fetched before the fork)
                ws = hip_ops.inbatch_fused_workspace(qi.shape[0], stack_q.out_dim, qi.device)

            def tower(i):
                acts = stacks[i].forward_acts(xs[i], flats[i], step=tsteps[i])
                if ws is not None:
                    hip_ops.inbatch_prep(acts[-1], i, logq if i else None, ws)
                return acts

            qa, ca = _both_towers(ctx.fork(qi), qi.device, tower)
        # cosine scoring: the loss entries run unchanged on the normalised
        # outputs (one launch for both), and its gradients are taken back to
        # the un-normalised ones after it (one launch, in place)
        q, c, invs = normalized_outputs(stack_q, stack_c, qa[-1], ca[-1])
        loss, dq, dc = stage(q, c, ws, functools.partial(unnormalize_grads, stack_q, stack_c, qa[-1], ca[-1], invs))
        ctx.stacks, ctx.nq, ctx.k = stacks, len(qa), len(cfg)
        ctx.save_for_backward(flat_q, flat_c, dq, dc, *qa, *ca)
        return loss

    @staticmethod
    def backward(ctx, g):
        flat_q, flat_c, dq, dc, *acts = ctx.saved_tensors
        stacks, flats, gouts, acts = ctx.stacks, (flat_q, flat_c), (dq, dc), (acts[:ctx.nq], acts[ctx.nq:])
        s = (g * ctx.scale if ctx.scale != 1.0 else g).reshape(1).float().contiguous()
        on_tower, on_dx, tsteps = _hooks(ctx.step)
        if ctx.pair:  # (on_dx unused: on_tower then applies each tower's whole update)
            (gqi, gflat_q), (gci, gflat_c) = backward_acts_pair(stacks, acts, flats, gouts, s,
                                                                ctx.needs_input_grad[:2])
            if on_tower is not None:  # the candidate tower's in its workspace scope (where its update was prepared)
                with hip_ops.Workspace.scope(TOWER_C_SCOPE):
                    on_tower(1, gci, gflat_c)
                on_tower(0, gqi, gflat_q)
        else:
            def tower(i):
                # this tower's updates (on_dx: the embedding update once its input gradient exists;
                # on_tower: the rest), the candidate tower's beside the query tower's backward
                out = stacks[i].backward_acts(acts[i], flats[i], gouts[i], s, ctx.needs_input_grad[i],
                                              on_dx=functools.partial(on_dx, i) if on_dx is not None else None,
                                              step=tsteps[i])
                if on_tower is not None:
                    on_tower(i, *out)
                return out

            (gqi, gflat_q), (gci, gflat_c) = _both_towers(ctx.fork(dq), dq.device, tower)
        return (gqi, gci, gflat_q, gflat_c) + (None,) * ctx.k


def global_inbatch_grads(q: torch.Tensor, c: torch.Tensor, logq: Optional[torch.Tensor], comm,
                         rows=None, cols=None, x3: Optional[bool] = None, ids: Optional[torch.Tensor] = None,
                         weights: Optional[torch.Tensor] = None, fold=None,
                         num_hard_negatives: Optional[int] = None, threshold=None):
    """This rank's share of the in-batch loss over the GLOBAL batch
    (two_tower_model.py:113-122 with the batch split over the ranks: row i's
    negatives are every candidate of every rank).  q, c: this rank's [b, E]
    rows (global rows rank*b ...); comm: all_gather over the ranks (equal b
    everywhere).  Returns (row_loss [b], dq [b, E], dc [b, E]): the loss
    terms of this rank's rows, d loss / d q of its rows, and d (global loss)
    / d c of its candidates.  The rows pass scores the local queries against
    all candidates; the cols pass scores all queries (with their lse) against
    the local candidates, so every gradient is summed inside one kernel in a
    fixed order (no cross-rank reduction of partial sums).  x3: fp32-faithful
    products in the library's entries (None: x3_scores(), the flag read at
    this call); injected rows / cols are called as they are.  ids: this
    rank's [b] int32 candidate ids — accidental hits removed over the global
    batch: the ids are all-gathered once, and the gathered vector is the rows
    pass's col_ids and the cols pass's row_ids (injected rows / cols receive
    row_ids / col_ids as keywords).  weights: this rank's [b] normalised
    sample weights (normalised by the GLOBAL w_max, which the caller puts
    into its loss scale) — the fold runs on the rank's own rows right after
    the rows pass (fold(w, lse, row_loss, dq) -> (lse_w, row_loss_w, wloss),
    dq scaled in place; hip_ops.inbatch_weight_rows unless injected), the
    all-gather of [lse, row_loss] then carries the folded values and nothing
    else moves; the first value returned is then wloss, the weighted terms.
    The one-rank shortcut through the single-device entry is not taken.
    num_hard_negatives: hard-negative mining over the global batch — the
    selection runs on this rank's rows against the gathered columns
    (threshold(q, C, L, k, pos_offset=off[, row_ids, col_ids]) -> thr [b];
    hip_ops.inbatch_hard_threshold unless injected), the rows pass takes thr=
    as a keyword, thr joins the all-gather of [lse, row_loss] as a third
    column, and the cols pass takes every row's thr= (injected rows / cols
    receive it as a keyword)."""
    if c.shape[0] != q.shape[0]:
        raise NotImplementedError(f"global_inbatch_grads: c has {c.shape[0]} rows for {q.shape[0]} rows of q; extra "
                                  "negatives (mixed negative sampling) are single-device only")
    if x3 is None:
        x3 = x3_scores()
    hard = _check_hard(num_hard_negatives)
    if (WORLD1_FUSED and weights is None and comm.world == 1 and rows is None and cols is None
            and threshold is None and not getattr(comm, "always", False)):
        # one rank: its rows are every row and its columns every column — the
        # single-device entry (one shared preparation of q and c for both passes)
        return _fused_grads(q, c, logq, ids, hard, x3)[:3]
    if hard is not None and threshold is None:
        threshold = functools.partial(hip_ops.inbatch_hard_threshold, x3=x3)
    rows = rows or (functools.partial(hip_ops.inbatch_rows, x3=True) if x3 else hip_ops.inbatch_rows)
    cols = cols or (functools.partial(hip_ops.inbatch_cols, x3=True) if x3 else hip_ops.inbatch_cols)
    b = q.shape[0]
    off = comm.rank * b
    C = comm.all_gather(c)                                     # [G b, E]
    L = comm.all_gather(logq) if logq is not None else None   # [G b]
    if ids is not None:
        I = comm.all_gather(ids)                               # [G b]: every candidate's id
        rows = functools.partial(rows, row_ids=ids, col_ids=I)
        cols = functools.partial(cols, row_ids=I, col_ids=ids)
        if hard is not None:
            threshold = functools.partial(threshold, row_ids=ids, col_ids=I)
    if hard is not None:
        thr = threshold(q, C, L, hard, pos_offset=off)         # [b]: this rank's rows against every column
        rows = functools.partial(rows, thr=thr)
    lse, row_loss, dq = rows(q, C, L, pos_offset=off)
    if weights is not None:
        lse, row_loss_w, wloss = (fold or hip_ops.inbatch_weight_rows)(weights, lse, row_loss, dq)
    Qa = comm.all_gather(q)                                    # [G b, E]
    # every row's scalars for the cols pass: lse, loss and, when mining, thr
    per_row = [lse, row_loss if weights is None else row_loss_w] + ([thr] if hard is not None else [])
    if comm.world > 1 or getattr(comm, "always", False):  # (one rank: its rows are every row, no stack / split copies)
        st = comm.all_gather(torch.stack(per_row[:2] + [t.to(lse.dtype) for t in per_row[2:]], 1))  # [G b, 2 or 3]
        per_row = [st[:, i].contiguous() for i in range(len(per_row))]
    if hard is not None:
        cols = functools.partial(cols, thr=per_row[2])
    dc = cols(Qa, per_row[0], c, logq, pos_offset=off, row_loss=per_row[1])  # local columns, every row
    return (row_loss if weights is None else wloss), dq, dc


def global_towers_inbatch_softmax_xent(qi: torch.Tensor, ci: torch.Tensor, stack_q, stack_c, comm,
                                       logq: Optional[torch.Tensor] = None,
                                       ids: Optional[torch.Tensor] = None,
                                       weights: Optional[torch.Tensor] = None,
                                       weight_scale: float = 1.0,
                                       num_hard_negatives: Optional[int] = None) -> torch.Tensor:
    """towers_inbatch_softmax_xent with the negatives of every rank
    (global_inbatch_grads; SUM reduction, the reference's runner.py:78-83):
    the returned loss is this rank's rows' share; the step sums it (and the
    gradients) over the ranks.  ids: this rank's candidate ids (accidental
    hits removed over the global batch).  weights: this rank's normalised
    sample weights, weight_scale the global w_max.  num_hard_negatives: hard
    negatives mined over the global batch.  Two streams from
    GLOBAL_TOWER_STREAMS rows."""
    hard = _check_hard(num_hard_negatives)
    scale = 1.0 * float(weight_scale) if weights is not None else 1.0

    def stage(q, c, ws, unnormalize):
        row_loss, dq, dc = global_inbatch_grads(q, c, logq, comm, ids=ids, weights=weights, num_hard_negatives=hard)
        unnormalize(dq, dc)
        return hip_ops.loss_sum(row_loss, scale), dq, dc

    return _TowersInBatchXent.apply(qi, ci, stack_q.flat, stack_c.flat, logq, stack_q, stack_c, scale, stage,
                                    _two_streams, False, None)


def towers_inbatch_softmax_xent(qi: torch.Tensor, ci: torch.Tensor, stack_q, stack_c,
                                logq: Optional[torch.Tensor] = None, reduction: str = "sum",
                                on_tower=None, on_dx=None, ids: Optional[torch.Tensor] = None,
                                weights: Optional[torch.Tensor] = None, weight_scale: float = 1.0,
                                num_hard_negatives: Optional[int] = None, *, step=None) -> torch.Tensor:
    """Loss of the query tower on qi against the candidate tower on ci (tower
    inputs [B, *]), fused into one autograd node; stack_* are DenseStacks.
    on_tower(i, input_grad, flat_grad), if given, is called in the backward as
    soon as tower i's (0 query, 1 candidate) gradients exist, on the stream and
    workspace scope they were produced in (the fused train step applies the
    optimizer there).  ids [B] (int32): accidental hits removed.  weights [B]
    (fp32, in [0, 1]) and weight_scale: sample weights (see above).
    num_hard_negatives: hard-negative mining (see above).  step: a train
    step's state (TwoTowerModel.TrainStep), which then brings the callbacks."""
    if reduction not in ("sum", "sum_over_batch_size", "mean"):
        raise ValueError(f"unsupported reduction {reduction}")
    hard = _check_hard(num_hard_negatives)
    scale = 1.0 if reduction == "sum" else 1.0 / qi.shape[0]
    if weights is not None:
        scale = scale * float(weight_scale)  # w_max: the loss is linear in w
    if step is None and (on_tower is not None or on_dx is not None):
        step = types.SimpleNamespace(on_tower=on_tower, on_dx=on_dx, towers=(None, None))
    # SPLIT_PREP: not under x3_scores() or with ids: those entries prepare their operands themselves;
    # not with normalised outputs: it would prepare the un-normalised ones
    split_prep = (SPLIT_PREP and not x3_scores() and ids is None and weights is None and hard is None
                  and not (stack_q.normalize or stack_c.normalize) and qi.shape[0] == ci.shape[0])

    def stage(q, c, ws, unnormalize):
        if weights is not None:  # sample weights: rows, fold, cols, tt_sum (either arithmetic, with or without ids)
            wloss, dq, dc = weighted_inbatch_grads(q, c, logq, weights, ids, num_hard_negatives=hard)
            loss = hip_ops.loss_sum(wloss, scale)
        else:  # (ws: only the plain bf16 loss has its operands prepared on the towers' streams)
            _, dq, dc, loss = _fused_grads(q, c, logq, ids, hard, x3_scores(), loss_scale=scale, ws=ws)
        unnormalize(dq, dc)
        return loss, dq, dc

    return _TowersInBatchXent.apply(qi, ci, stack_q.flat, stack_c.flat, logq, stack_q, stack_c, scale, stage,
                                    lambda x: x.is_cuda, split_prep, step)


def inbatch_softmax_xent(q: torch.Tensor, c: torch.Tensor, logq: Optional[torch.Tensor] = None,
                         reduction: str = "sum", ids: Optional[torch.Tensor] = None,
                         weights: Optional[torch.Tensor] = None, weight_scale: float = 1.0,
                         num_hard_negatives: Optional[int] = None) -> torch.Tensor:
    """Loss of query rows q [B,E] against candidates c [B,E] (positive of row
    i is column i), logq [B] the per-candidate log sampling probability.
    c [B + M, E]: rows past B are extra negatives of every row (see above).
    ids [B] (int32): accidental hits removed (see above).  weights [B] (fp32,
    in [0, 1]) and weight_scale: sample weights (see above).
    num_hard_negatives: hard-negative mining (see above)."""
    if reduction not in ("sum", "sum_over_batch_size", "mean"):
        raise ValueError(f"unsupported reduction {reduction}")
    scale = 1.0 if reduction == "sum" else 1.0 / q.shape[0]
    hard = _check_hard(num_hard_negatives)
    if not q.requires_grad and not c.requires_grad:
        # the scores the training loss is computed from, in either mode
        kw = {"x3": x3_scores(), "row_ids": _row_ids(ids, q, c), "col_ids": ids}  # (extra negatives: the rows entries as they are)
        if hard is not None:
            kw["thr"] = hip_ops.inbatch_hard_threshold(q, c, logq, hard, **kw)
        lse, row_loss, _ = hip_ops.inbatch_rows(q, c, logq, want_dq=False, **kw)
        if weights is not None:
            _, _, wloss = hip_ops.inbatch_weight_rows(weights, lse, row_loss)
            return hip_ops.loss_sum(wloss, scale * weight_scale)
        return hip_ops.loss_sum(row_loss, scale)
    return _InBatchXent.apply(q, c, logq, scale, ids, weights, float(weight_scale), hard)


class InBatchSoftmaxCrossEntropy:
    """Stand-in for tf.keras.losses.CategoricalCrossentropy(from_logits=True,
    reduction=SUM) as compiled by the reference runner (runner.py:78-83)."""

    def __init__(self, from_logits: bool = True, reduction: str = "sum"):
        if not from_logits:
            raise ValueError("the in-batch loss is defined on logits (from_logits=True)")
        self.reduction = str(reduction).lower().split(".")[-1]

    def __call__(self, q, c, logq=None, ids=None, weights=None, weight_scale: float = 1.0, num_hard_negatives=None):
        return inbatch_softmax_xent(q, c, logq, self.reduction, ids, weights, weight_scale, num_hard_negatives)


# Name the reference compiles with.
CategoricalCrossentropy = InBatchSoftmaxCrossEntropy
