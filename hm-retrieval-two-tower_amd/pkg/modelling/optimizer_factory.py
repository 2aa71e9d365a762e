"""Optimizers with tf.keras.optimizers.legacy semantics, applied by libtt.

Mirror of /root/reference/pkg/modelling/optimizer_factory.py:8-57 (same names,
same required kwargs and error messages).  The update rules are the legacy
Keras / TF kernels the reference reaches:
  Adagrad (initial_accumulator_value=0.1, epsilon=1e-7):
    dense  ResourceApplyAdagradV2        -> tt_dense_adagrad (one launch per tower)
    sparse dedup + ResourceSparseApplyAdagradV2 -> tt_sparse_adagrad
  Adam (beta_1=0.9, beta_2=0.999, epsilon=1e-7):
    dense  ResourceApplyAdam             -> tt_dense_adam
    sparse legacy _resource_apply_sparse (decays the WHOLE m/v slots, then a
           dense var update)              -> tt_sparse_adam
    with the step count on the device (Adam.enable_device_clock, what a
    captured step needs): tt_adam_clock_advance, then tt_dense_adam_many_dev
    and tt_sparse_adam_dev, the same arithmetic with the step's coefficients
    read from the device clock
Slots are created on first use, as Keras creates them on the first
apply_gradients.
Both take the legacy keywords clipvalue, clipnorm and global_clipnorm
(_transform_gradients: clamp, then a per-variable or a global norm bound),
applied in place on the device before any update: _Optimizer.clip_gradients ->
tt_grad_sumsq, tt_grad_clip_apply.  decay is refused.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple
import logging
import math

import torch

from pkg.modelling import hip_ops

logger = logging.getLogger(__name__)

__all__ = ["OptimizerFactory", "Adagrad", "Adam", "plan_clip_regions", "clip_tower_desc"]


CLIP_KEYS = ("clipvalue", "clipnorm", "global_clipnorm")


def plan_clip_regions(towers: Sequence[dict]) -> Tuple[List[str], List[dict]]:
    """The variables Keras clips as one tensor each, and where their gradient
    values lie.  Pure Python (no tensor is touched).  Each tower is a dict:
      name      prefix of its variables' names
      layout    DenseStack.layout, [(w_off, fan_in, fan_out, b_off)]; [] when
                the tower has no dense gradient this step
      rows      rows of its input gradient (B, or B + M for the candidate
                tower under mixed negatives); None when it has none
      features  its categorical lookups in call order, (table name, dim,
                column offset, L): L None for a one-id lookup, the sequence
                length for a sequence feature
    Variables, in order, per tower: every Dense layer's kernel then bias, then
    every embedding table at its first lookup (a name looked up twice is ONE
    variable with several regions).  Numeric columns belong to no variable.
    Returns (names, regions); a region is a dict with var, tower and
      kind "dense": start, size      flat.grad[start : start + size]
      kind "input": col, cols, rows  last_grad[:, col : col + cols]
      kind "bag":   bag, cols, rows  the expanded G of the tower's bag-th
                                     sequence feature, rows of valid slots only"""
    names: List[str] = []
    regions: List[dict] = []
    for ti, t in enumerate(towers):
        for li, (w_off, fi, fo, b_off) in enumerate(t["layout"]):
            for what, start, size in (("kernel", w_off, fi * fo), ("bias", b_off, fo)):
                regions.append(dict(var=len(names), tower=ti, kind="dense", start=start, size=size))
                names.append(f"{t['name']}/dense_{li}/{what}")
        var_of: Dict[str, int] = {}
        bag = 0
        for table, dim, col, L in t["features"]:
            if table not in var_of:
                var_of[table] = len(names)
                names.append(f"{t['name']}/embedding/{table}")
            rows = t["rows"]
            if L is None:
                if rows is not None:
                    regions.append(dict(var=var_of[table], tower=ti, kind="input", col=col, cols=dim, rows=rows))
            else:
                if rows is not None:
                    regions.append(dict(var=var_of[table], tower=ti, kind="bag", bag=bag, cols=dim, rows=rows * L))
                bag += 1
    return names, regions


def clip_tower_desc(tower, name: str, rows: Optional[int], dense: bool = True) -> dict:
    """plan_clip_regions' description of a Tower (its structure; `rows` and
    `dense` say which gradients this step has)."""
    layer = tower.input_layer
    features = [(f.name, layer.embedding_layers[f.name].dim, off, f.sequence_length if f.is_sequence else None)
                for f, off in zip(layer.categorical_features, layer.column_offsets())]
    return dict(name=name, layout=list(tower.dense.layout) if dense else [], rows=rows, features=features)


class _Optimizer:
    def __init__(self, learning_rate: float = 0.001, name: str = "", **kwargs):
        self.learning_rate = float(learning_rate)
        self.name = name
        self.iterations = 0
        self._slots: Dict[int, List[torch.Tensor]] = {}
        unknown = set(kwargs) - set(CLIP_KEYS) - {"decay"}
        if unknown:
            raise TypeError(f"Unexpected keyword argument(s) passed to optimizer: {sorted(unknown)}")
        if kwargs.get("decay"):
            raise NotImplementedError("decay is not supported")
        for k in CLIP_KEYS:
            v = kwargs.get(k)
            if v is not None:
                if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
                    raise ValueError(f"{k} must be None or a positive finite number, got {v!r}")
                v = float(v)
            setattr(self, k, v)
        if self.clipnorm is not None and self.global_clipnorm is not None:
            raise ValueError("Cannot accept both `clipnorm` and `global_clipnorm`, "
                             f"got clipnorm={self.clipnorm}, global_clipnorm={self.global_clipnorm}")
        self.clips = any(getattr(self, k) is not None for k in CLIP_KEYS)
        self.clip_variable_names: List[str] = []
        self._clip_state = None  # (num_vars, device, sumsq fp64, factor fp32): persistent, a captured step replays into them
        self._clip_bags: Dict[int, list] = {}

    # -- gradient clipping (clipvalue, clipnorm, global_clipnorm) --------------
    TOWER_NAMES = ("query", "candidate")

    @property
    def last_clip_sumsq(self) -> Optional[torch.Tensor]:
        """Per variable (clip_variable_names), the fp64 sum of squares of its
        gradient values after clipvalue, of the last clip_gradients; None
        before the first one and with neither norm set.  A device tensor:
        reading it is the caller's synchronisation."""
        if self._clip_state is None or (self.clipnorm is None and self.global_clipnorm is None):
            return None
        return self._clip_state[2]

    @property
    def last_clip_factors(self) -> Optional[torch.Tensor]:
        """Per variable, the fp32 factor the last clip_gradients applied (1
        where the norm did not exceed its bound; one value for all under
        global_clipnorm)."""
        return None if self._clip_state is None else self._clip_state[3]

    def clip_gradients(self, towers) -> None:
        """Keras' _transform_gradients on the device, in place, before any
        update: clipvalue, then clipnorm per variable or global_clipnorm over
        all (plan_clip_regions says what a variable is).  Sequence features'
        gradients are expanded here, clipped as the rows the bag applies
        consume, and handed to them (_apply_bags).  Launches on the current
        stream, no host read; nothing is launched without a clipping keyword."""
        if not self.clips:
            return
        names, regions = self._clip_regions(towers)
        if not regions:
            return
        device = regions[0][0].device
        st = self._clip_state
        if st is None or st[0] != len(names) or st[1] != device:
            st = self._clip_state = (len(names), device, torch.zeros(len(names), dtype=torch.float64, device=device),
                                     torch.ones(len(names), dtype=torch.float32, device=device))
        self.clip_variable_names = names
        arr = hip_ops.clip_regions(regions, len(names))
        norm = self.clipnorm is not None or self.global_clipnorm is not None
        if norm:
            hip_ops.grad_sumsq(arr, len(names), self.clipvalue, st[2])
        hip_ops.grad_clip_apply(arr, len(names), self.clipvalue, self.clipnorm, self.global_clipnorm,
                                st[2] if norm else None, st[3])

    def _clip_regions(self, towers) -> Tuple[List[str], List[tuple]]:
        """plan_clip_regions for this step's gradients, bound to their tensors:
        (variable names, [(g, row_ids or None, var)] for hip_ops.clip_regions).
        Expands the towers' bag gradients (kept for _apply_bags)."""
        descs, expanded = [], []
        self._clip_bags = {}
        for ti, tower in enumerate(towers):
            layer, g = tower.input_layer, tower.input_layer.last_grad
            bags = []
            if g is not None and layer.bag_sources():
                # one buffer per tower: every tower's G is alive until the norm is known
                bags = self._expand_bags(tower, g, tag=f"bag_grad_clip{ti}")
                self._clip_bags[id(tower)] = bags
            expanded.append(bags)
            name = self.TOWER_NAMES[ti] if len(towers) == len(self.TOWER_NAMES) else f"tower{ti}"
            descs.append(clip_tower_desc(tower, name, None if g is None else g.shape[0],
                                         dense=tower.dense.flat.grad is not None))
        names, plan = plan_clip_regions(descs)
        regions = []
        for r in plan:
            tower = towers[r["tower"]]
            if r["kind"] == "dense":
                regions.append((tower.dense.flat.grad[r["start"]:r["start"] + r["size"]], None, r["var"]))
            elif r["kind"] == "input":
                regions.append((tower.input_layer.last_grad[:, r["col"]:r["col"] + r["cols"]], None, r["var"]))
            else:
                _, _, ids_flat, G = expanded[r["tower"]][r["bag"]]
                regions.append((G, ids_flat, r["var"]))
        return names, regions

    def _slot(self, param: torch.Tensor, n: int, init: float) -> List[torch.Tensor]:
        key = id(param)
        s = self._slots.get(key)
        if s is None or s[0].shape != param.shape:
            s = [torch.full_like(param, init, requires_grad=False) for _ in range(n)]
            self._slots[key] = s
        return s

    def apply_gradients(self, towers) -> None:
        """Dense step on each tower's flat MLP buffer, sparse step on its tables."""
        self._apply(towers)
        self.iterations += 1

    minimize = apply_gradients

    # -- sequence features: a tower's bag tables as flat sparse problems -------
    BAG_WS_TAG = "sparse_bag"  # the regular tables' presorted keys may sit in "sparse"

    def _expand_bags(self, tower, grad: torch.Tensor, tag: str = "bag_grad") -> list:
        """One gradient row per lookup of the tower's sequence features (ONE
        tt_bag_grad_expand launch per 8 features), carved from the workspace
        `tag`: [(L, table, ids_flat [B * L], G [B * L, dim])] per feature."""
        bags = tower.input_layer.bag_sources()
        if grad.stride(1) != 1:
            grad = grad.contiguous()
        B = grad.shape[0]
        sizes = [(B * b["ids"].shape[1], b["table"].dim) for b in bags]
        offs, total = [], 0
        for n, dim in sizes:  # 256-byte aligned carves: ids_flat then G per feature
            offs.append((total, total + (n * 4 + 255) // 256 * 256))
            total = offs[-1][1] + (n * dim * 4 + 255) // 256 * 256
        buf = hip_ops.Workspace.get(total, grad.device, tag)
        jobs, out = [], []
        for b, (n, dim), (o_ids, o_g) in zip(bags, sizes, offs):
            ids_flat = buf[o_ids:o_ids + n * 4].view(torch.int32)
            G = buf[o_g:o_g + n * dim * 4].view(torch.float32).view(n, dim)
            t = b["table"]
            jobs.append((t.num_rows, b["ids"], b["pooling"], grad, b["grad_col_offset"], b["scale"], ids_flat, G))
            out.append((b["ids"].shape[1], t, ids_flat, G))
        for i in range(0, len(jobs), hip_ops._native.MAX_BAG_JOBS):
            hip_ops.bag_grad_expand(jobs[i:i + hip_ops._native.MAX_BAG_JOBS], B)
        return out

    def _apply_bags(self, tower, grad: Optional[torch.Tensor], apply) -> None:
        """Expand the tower's input gradient into one gradient row per lookup of
        its sequence features (ONE tt_bag_grad_expand launch per 8 features) and
        hand every group of equal L to `apply(specs, batch * L, G)` as a flat
        problem: one source per table, ids_flat, grad_ld = dim, column 0.  On
        the current stream and workspace scope, after the tower's regular
        sparse call; nothing is launched without a sequence feature.  After
        clip_gradients the rows it expanded (and clipped) are applied instead."""
        expanded = self._clip_bags.pop(id(tower), None)
        if expanded is None:
            if not tower.input_layer.bag_sources() or grad is None:
                return
            expanded = self._expand_bags(tower, grad)
        by_len = {}
        for L, t, ids_flat, G in expanded:
            by_len.setdefault(L, []).append((t, ids_flat, G))
        for group in by_len.values():  # tables of different L take separate calls
            apply(group, group[0][1].numel())


class Adagrad(_Optimizer):
    def __init__(self, learning_rate: float = 0.001, initial_accumulator_value: float = 0.1, epsilon: float = 1e-7,
                 name: str = "Adagrad", **kwargs):
        super().__init__(learning_rate, name, **kwargs)
        if initial_accumulator_value < 0.0:
            raise ValueError(f"initial_accumulator_value must be non-negative: {initial_accumulator_value}")
        self.initial_accumulator_value = float(initial_accumulator_value)
        self.epsilon = float(epsilon)
        self._prepared = None
        self._side_streams = {}

    def _sparse_specs(self, towers, with_grad: bool, grad: Optional[torch.Tensor] = None):
        init = self.initial_accumulator_value
        specs, batch = [], None
        for tower in towers:
            layer = tower.input_layer
            if not layer.embedding_layers:
                continue
            g = grad if grad is not None else layer.last_grad
            if with_grad and g is None:
                continue
            for src in layer.sparse_sources():
                t = src["table"]
                (acc,) = self._slot(t.weight, 1, init)
                batch = src["ids"][0].numel()
                specs.append(dict(table=t.weight, slot0=acc, ids=src["ids"], grad_col_offset=src["grad_col_offset"],
                                  grad=g if with_grad else None))
        return specs, batch

    # -- per-tower application from inside the backward (TwoTowerModel.train_step)
    def prepare_towers(self, towers, scopes: List[str]) -> None:
        """One id sort per tower (tower i's workspace scope scopes[i]) on the
        side stream, before the backward, so each tower's update can be applied
        by apply_tower the moment that tower's gradients exist."""
        self._tower_prep = {}
        if not torch.cuda.is_available():
            return
        cur = torch.cuda.current_stream()
        side = self._side_streams.get(cur.device)
        if side is None:
            side = self._side_streams[cur.device] = torch.cuda.Stream(device=cur.device)
        side.wait_stream(cur)
        for tower, scope in zip(towers, scopes):
            with torch.cuda.stream(side), hip_ops.Workspace.scope(scope):
                specs, batch = self._sparse_specs([tower], with_grad=False)  # new accumulators filled on `side`
                if not specs or len(specs) > 16 or not batch:
                    # not presorted: apply_tower sorts on the current stream,
                    # which must first see the accumulators filled on `side`
                    if specs:
                        cur.wait_stream(side)
                    continue
                hip_ops.sparse_sort(specs, batch)
                key = hip_ops.Workspace._scope  # the apply must find its sorted keys in this scope's buffer
            done = torch.cuda.Event()
            done.record(side)
            self._tower_prep[id(tower)] = ([id(s["table"]) for s in specs], batch, done, key)

    def apply_dense(self, tower, flat_grad: torch.Tensor) -> None:
        """Tower's dense Adagrad step alone, on the current stream (the same
        update _apply makes from flat.grad)."""
        flat = tower.dense.flat
        (acc,) = self._slot(flat, 1, self.initial_accumulator_value)
        hip_ops.dense_adagrad(flat.data, acc, flat_grad, self.learning_rate, self.epsilon)

    def apply_tower(self, tower, input_grad: Optional[torch.Tensor], flat_grad: torch.Tensor) -> None:
        """Tower's dense Adagrad step and its tables' sparse step, on the current
        stream and workspace scope (the ones prepare_towers used for it)."""
        self.apply_dense(tower, flat_grad)
        self.apply_tower_sparse(tower, input_grad)

    def _apply_bag_group(self, group, batch: int) -> None:
        specs = []
        for t, ids_flat, G in group:
            (acc,) = self._slot(t.weight, 1, self.initial_accumulator_value)
            specs.append(dict(table=t.weight, slot0=acc, ids=[ids_flat], grad_col_offset=[0], grad=G))
        hip_ops.sparse_adagrad(specs, batch, None, self.learning_rate, self.epsilon, ws_tag=self.BAG_WS_TAG)

    def apply_tower_sparse(self, tower, input_grad: Optional[torch.Tensor]) -> None:
        """Tower's tables' sparse Adagrad step alone (apply_tower's second
        half), on the current stream and workspace scope; its sequence
        features' tables follow the regular call."""
        self._apply_tower_tables(tower, input_grad)
        self._apply_bags(tower, input_grad, self._apply_bag_group)

    def _apply_tower_tables(self, tower, input_grad: Optional[torch.Tensor]) -> None:
        lr, eps = self.learning_rate, self.epsilon
        prep = getattr(self, "_tower_prep", {}).pop(id(tower), None)
        if input_grad is None:
            return
        specs, batch = self._sparse_specs([tower], with_grad=True, grad=input_grad)
        if not specs:
            return
        if prep is None:  # prepare_towers skipped this tower: sort here
            hip_ops.sparse_adagrad(specs, batch, None, lr, eps)
            return
        torch.cuda.current_stream().wait_event(prep[2])
        if (prep[0] != [id(s["table"]) for s in specs] or prep[1] != batch
                or prep[3] != hip_ops.Workspace._scope):
            raise RuntimeError(f"apply_tower: presorted state {prep[0]}/{prep[1]}/{prep[3]!r} does not match "
                               f"this apply ({[id(s['table']) for s in specs]}/{batch}/{hip_ops.Workspace._scope!r})")
        hip_ops.sparse_adagrad(specs, batch, None, lr, eps, presorted=True)

    def prepare(self, towers, after: Optional[torch.cuda.Event] = None) -> None:
        """Start the embedding update's id sort early, on a side stream (it reads
        only the lookup ids of the last gather), so it overlaps the backward
        pass; apply_gradients then joins it.  `after`: an event of the current
        stream the sort must follow (default: everything queued so far).
        Optional: without it the sort runs inside apply_gradients."""
        self._prepared = None
        if not torch.cuda.is_available():
            return
        cur = torch.cuda.current_stream()
        side = self._side_streams.get(cur.device)
        if side is None:
            side = self._side_streams[cur.device] = torch.cuda.Stream(device=cur.device)
        if after is not None:
            side.wait_event(after)  # ordered after that point of this stream only
        else:
            side.wait_stream(cur)
        with torch.cuda.stream(side):
            # accumulators created here are filled on this stream, ahead of
            # anything ordered after the sort
            specs, batch = self._sparse_specs(towers, with_grad=False)
            # (towers on different batches — mixed negative sampling runs the
            # candidate tower on B + M rows — are sorted and applied per tower
            # by _apply, not presorted here)
            if not specs or len(specs) > 16 or not batch or not self._one_batch(specs):
                if specs:  # the apply sorts on `cur`: order it after the accumulator fills
                    cur.wait_stream(side)
                return
            hip_ops.sparse_sort(specs, batch)
        done = torch.cuda.Event()
        done.record(side)
        self._prepared = ([id(s["table"]) for s in specs], batch, done)

    @staticmethod
    def _one_batch(specs) -> bool:
        """True when every table of `specs` was looked up with the same batch."""
        return len({s["ids"][0].numel() for s in specs}) <= 1

    def _apply(self, towers) -> None:
        lr, eps, init = self.learning_rate, self.epsilon, self.initial_accumulator_value
        self.clip_gradients(towers)
        for tower in towers:
            flat = tower.dense.flat
            if flat.grad is not None:
                (acc,) = self._slot(flat, 1, init)
                hip_ops.dense_adagrad(flat.data, acc, flat.grad, lr, eps)
        specs, batch = self._sparse_specs(towers, with_grad=True)
        prepared, self._prepared = self._prepared, None
        if prepared is not None:  # join the side stream before anything touches the workspace
            torch.cuda.current_stream().wait_event(prepared[2])
        if specs and not self._one_batch(specs):
            # the towers' batches differ: one sort and one apply per tower
            for tower in towers:
                tspecs, tbatch = self._sparse_specs([tower], with_grad=True)
                if tspecs:
                    hip_ops.sparse_adagrad(tspecs, tbatch, None, lr, eps)
        elif specs:
            # every tower's tables in ONE call: one sort, one block pass (each
            # table reads its own tower's input gradient)
            if prepared is None:
                hip_ops.sparse_adagrad(specs, batch, None, lr, eps)
            elif prepared[0] == [id(s["table"]) for s in specs] and prepared[1] == batch:
                hip_ops.sparse_adagrad(specs, batch, None, lr, eps, presorted=True)
            else:
                raise RuntimeError(f"apply_gradients: presorted state {prepared[0]}/{prepared[1]} does not match "
                                   f"this apply ({[id(s['table']) for s in specs]}/{batch})")
        for tower in towers:
            self._apply_bags(tower, tower.input_layer.last_grad, self._apply_bag_group)

    def check_status(self, device: Optional[torch.device] = None) -> None:
        """Raise if any sparse apply since the last check found keys that were
        not its call's (libtt records it on the device instead of applying;
        tt_sparse_status).  Synchronises the current stream."""
        from pkg.modelling.losses import TOWER_C_SCOPE

        if not torch.cuda.is_available():
            return
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        for scope in ("", TOWER_C_SCOPE):
            hip_ops.sparse_status(dev, "sparse", scope)
            hip_ops.sparse_status(dev, self.BAG_WS_TAG, scope)


class Adam(_Optimizer):
    def __init__(self, learning_rate: float = 0.001, beta_1: float = 0.9, beta_2: float = 0.999,
                 epsilon: float = 1e-7, amsgrad: bool = False, name: str = "Adam", **kwargs):
        super().__init__(learning_rate, name, **kwargs)
        if amsgrad:
            raise NotImplementedError("amsgrad is not supported")
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)

    # -- the step count: a host integer, or the device clock's word once enabled
    _clock: Optional[torch.Tensor] = None

    @property
    def iterations(self) -> int:
        """Steps applied so far.  With the device clock enabled this reads the
        clock's step word (it synchronises the current stream), so it counts
        eager steps and graph replays alike."""
        if self._clock is not None:
            return int(self._clock[0].item())
        return self._iterations

    @iterations.setter
    def iterations(self, value: int) -> None:
        self._iterations = int(value)
        if self._clock is not None:
            self._clock[:1].fill_(int(value))

    def enable_device_clock(self, device) -> None:
        """Move the step count into device memory (a tt_adam_clock), so a step
        can be captured in a graph and every replay is the next step.

        Builds, once, the table of both step coefficients from learning_rate,
        beta_1 and beta_2 with the host function the host-step entries use
        (tt_adam_coef_fill; the coefficients equal learning_rate from step
        tt_adam_coef_len on, where the table ends), uploads it and sets the
        clock's step to the current `iterations`.  learning_rate is read HERE:
        a later change of the attribute does not reach the table.  From then on
        every apply, eager or captured, is one adam_clock_advance, one
        dense_adam_many_dev and the sparse_adam_dev calls, with results equal to
        the host-step path's bit for bit, and the device word is the count
        `iterations` reports.  A second call is a no-op.  Raises ValueError for
        betas whose table cannot be built (beta = 1, or so close to 1 that it
        would pass 2^22 entries)."""
        if self._clock is not None:
            return
        length = hip_ops.adam_coef_len(self.beta_1, self.beta_2)
        if length == 0:
            raise ValueError(f"Adam's device step clock needs beta_1 and beta_2 in [0, 1) whose powers vanish in fp32 "
                             f"within 2^22 steps; got beta_1={self.beta_1}, beta_2={self.beta_2}")
        alpha, lr_t = hip_ops.adam_coef_tables(self.learning_rate, self.beta_1, self.beta_2, length)
        device = torch.device(device)
        self._coef_tables = (alpha.to(device), lr_t.to(device))
        clock = torch.zeros(2, dtype=torch.int64, device=device)
        clock[:1].fill_(self._iterations)
        self._clock = clock

    def apply_gradients(self, towers) -> None:
        if self._clock is None:
            return super().apply_gradients(towers)
        self._apply_dev(towers)  # its first launch advances the device's count

    minimize = apply_gradients

    def _apply_dev(self, towers) -> None:
        b1, b2, eps, clock = self.beta_1, self.beta_2, self.epsilon, self._clock
        self.clip_gradients(towers)
        hip_ops.adam_clock_advance(clock, *self._coef_tables)
        jobs = []
        for tower in towers:
            flat = tower.dense.flat
            if flat.grad is not None:
                m, v = self._slot(flat, 2, 0.0)
                jobs.append((flat.data, m, v, flat.grad))
        if jobs:  # both towers' MLP buffers in one launch
            hip_ops.dense_adam_many_dev(jobs, b1, b2, eps, clock)
        calls = []  # (specs, batch) per tower with an input gradient
        for tower in towers:
            layer = tower.input_layer
            if layer.last_grad is None or not layer.embedding_layers:
                continue
            specs = []
            for src in layer.sparse_sources():
                t = src["table"]
                m, v = self._slot(t.weight, 2, 0.0)
                specs.append(dict(table=t.weight, slot0=m, slot1=v, ids=src["ids"],
                                  grad_col_offset=src["grad_col_offset"], grad=layer.last_grad))
            if specs:
                calls.append((specs, layer.last_grad.shape[0]))
        if len({batch for _, batch in calls}) == 1:
            # every tower's tables in ONE call (each table reads its own tower's
            # input gradient): one sort, one decay launch, one update launch
            calls = [([s for specs, _ in calls for s in specs], calls[0][1])]
        for specs, batch in calls:  # batches differ (mixed negatives: B and B + M rows): one call per tower
            hip_ops.sparse_adam_dev(specs, batch, None, b1, b2, eps, clock)

        def apply_group(group, batch):
            bag_specs = []
            for t, ids_flat, G in group:
                m, v = self._slot(t.weight, 2, 0.0)
                bag_specs.append(dict(table=t.weight, slot0=m, slot1=v, ids=[ids_flat], grad_col_offset=[0], grad=G))
            hip_ops.sparse_adam_dev(bag_specs, batch, None, b1, b2, eps, clock, ws_tag=self.BAG_WS_TAG)

        for tower in towers:
            layer = tower.input_layer
            if layer.last_grad is not None and layer.embedding_layers:
                self._apply_bags(tower, layer.last_grad, apply_group)

    def _apply(self, towers) -> None:
        step = self.iterations + 1
        lr, b1, b2, eps = self.learning_rate, self.beta_1, self.beta_2, self.epsilon
        self.clip_gradients(towers)
        for tower in towers:
            flat = tower.dense.flat
            if flat.grad is not None:
                m, v = self._slot(flat, 2, 0.0)
                hip_ops.dense_adam(flat.data, m, v, flat.grad, lr, b1, b2, eps, step)
            layer = tower.input_layer
            if layer.last_grad is None or not layer.embedding_layers:
                continue
            specs = []
            for src in layer.sparse_sources():
                t = src["table"]
                m, v = self._slot(t.weight, 2, 0.0)
                specs.append(dict(table=t.weight, slot0=m, slot1=v, ids=src["ids"],
                                  grad_col_offset=src["grad_col_offset"]))
            if specs:
                hip_ops.sparse_adam(specs, layer.last_grad.shape[0], layer.last_grad, lr, b1, b2, eps, step)

            def apply_group(group, batch):
                bag_specs = []
                for t, ids_flat, G in group:
                    m, v = self._slot(t.weight, 2, 0.0)
                    bag_specs.append(dict(table=t.weight, slot0=m, slot1=v, ids=[ids_flat], grad_col_offset=[0],
                                          grad=G))
                hip_ops.sparse_adam(bag_specs, batch, group[0][2], lr, b1, b2, eps, step, ws_tag=self.BAG_WS_TAG)

            self._apply_bags(tower, layer.last_grad, apply_group)


class OptimizerFactory:
    """
    Fetch a supported optimizer instance using config.
    Some kwargs are required.
    """

    _supported_optimizers = {
        "adam": Adam,
        "adagrad": Adagrad,
    }

    _required_kwargs = ["learning_rate"]

    @classmethod
    def get_optimizer(cls, optimizer_name: str, optimizer_kwargs: Dict[str, Any]) -> _Optimizer:
        if optimizer_name not in cls._supported_optimizers:
            raise ValueError(
                "name must be one of "
                f"{list(cls._supported_optimizers.keys())}, "
                f"got {optimizer_name}"
            )
        for kwarg in cls._required_kwargs:
            if kwarg not in optimizer_kwargs:
                raise ValueError(f"kwarg {kwarg} not found in kwargs: {optimizer_kwargs}")
        logger.info(f"Creating {optimizer_name} obj with kwargs: {optimizer_kwargs}")
        return cls._supported_optimizers[optimizer_name](**optimizer_kwargs)
