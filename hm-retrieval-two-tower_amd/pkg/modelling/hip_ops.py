"""Torch-tensor wrappers over the libtt C ABI (include/tt.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream.
Every function checks shapes/dtypes/devices on the host, passes raw device
pointers plus torch's current stream to libtt, and raises on error.  There is
no CPU or eager fallback: a CPU tensor or a missing libtt.so is an error.
"""
from __future__ import annotations

import contextlib
import ctypes
import gc
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from pkg import _native
from pkg._native import GatherSegment, SparseTable, check, lib

__all__ = [
    "loss_sum",
    "gather_grouped",
    "sparse_adagrad",
    "sparse_adagrad_rows",
    "sparse_sort",
    "sparse_status",
    "sparse_adam",
    "dedup_sum",
    "dense_adagrad",
    "dense_adagrad_many",
    "dense_adam",
    "adam_coef_len",
    "adam_coef_tables",
    "adam_clock_advance",
    "dense_adam_many_dev",
    "sparse_adam_dev",
    "inbatch_rows",
    "inbatch_hard_threshold",
    "inbatch_cols",
    "inbatch_weight_rows",
    "inbatch_fused",
    "inbatch_fused_mixed",
    "mixed_candidates",
    "inbatch_fused_workspace",
    "inbatch_prep",
    "l2norm_rows",
    "l2norm_rows_grad",
    "gather_bag",
    "bag_grad_expand",
    "clip_regions",
    "grad_sumsq",
    "grad_clip_apply",
    "probe_arm",
    "probe_arm_repeat",
    "route_requests",
    "route_pad",
    "route_fixed",
    "sparse_routed",
    "route_owner",
    "bruteforce_build",
    "bruteforce_search",
    "bruteforce_shard_search",
    "topk_merge",
    "topk_exclude",
    "recall_hits",
    "rank_metrics",
    "rank_discount_tables",
    "Workspace",
    "capture_guard",
    "CaptureTopology",
    "NestedJoinError",
]


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _req(t: torch.Tensor, name: str, dtype: torch.dtype, ndim: Optional[int] = None) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must live on the GPU (got {t.device}); libtt has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name} must be {ndim}-D, got shape {tuple(t.shape)}")


def _row_major(t: torch.Tensor, name: str) -> int:
    """Leading dimension of a 2-D tensor with unit column stride."""
    if t.dim() != 2 or (t.stride(1) != 1 and t.shape[1] > 1 and t.numel() > 0):
        raise ValueError(f"{name} must be 2-D with unit column stride")
    # an empty tensor's strides carry no layout (numpy hands over zeros): nothing is read
    return max(t.stride(0), t.shape[1])


class NestedJoinError(RuntimeError):
    """A captured stream waited on a side branch without being the capture's
    origin stream (CaptureTopology)."""


class CaptureTopology:
    """The fork / join structure of one hipGraph capture, checked as it is
    issued.  ROCm 7.2's hipStreamEndCapture segfaults when a captured side
    branch waits on another side branch — the branch that forked it
    (tools/graph_fork_probe.py nested_join, profiles/r03_graph_fork_probe.txt)
    or a sibling (the round-5 embedding update on the id-sort stream) — so
    here only the capture's origin stream may wait on a branch; a stream
    entering the capture may wait on any captured stream (a fork) and a
    branch may wait on the origin again.  The origin is the stream of the first event
    recorded while capturing (nothing else is in the capture yet).  On a
    violating wait the wait is NOT issued: every branch is joined into the
    origin instead (so the capture can end cleanly) and NestedJoinError is
    raised."""

    def __init__(self):
        self.active = True
        self.depth = 0  # > 0 inside a checked Stream.wait_event (its Event.wait is the same wait)
        self.origin = None
        self.branches: Dict[int, object] = {}  # stream id -> stream (streams that joined by waiting)
        self.source: Dict[int, object] = {}    # id(event) -> stream it was recorded on

    def recorded(self, event, stream) -> None:
        if not self.active:
            return
        if self.origin is None:
            if not torch.cuda.is_current_stream_capturing():
                return
            self.origin = stream
        self.source[id(event)] = stream

    def waiting(self, stream, event) -> None:
        src = self.source.get(id(event)) if self.active else None
        if src is None or self.origin is None or src == stream:
            return
        if stream != self.origin and stream.cuda_stream not in self.branches:
            # a stream entering the capture: a fork (from the origin or from a
            # branch: legal, tools/graph_fork_probe.py origin_join)
            self.branches[stream.cuda_stream] = stream
            return
        if src != self.origin and stream != self.origin:
            origin, branches = self.origin, list(self.branches.values())
            self.active = False  # the repair below is not itself checked, nor anything after it
            for b in branches:
                origin.wait_stream(b)
            raise NestedJoinError(
                f"captured stream {stream} waits on side branch {src}: only the capture's origin stream "
                f"({origin}) may join a branch (ROCm's hipStreamEndCapture crashes on nested joins)")


@contextlib.contextmanager
def capture_guard(keep: Optional[list] = None):
    """Around a hipGraph capture on this thread: Python's garbage collector
    off (collected first) — a collection mid-capture can run a finalizer that
    frees device or pinned host memory or destroys an event, which the
    runtime refuses during capture and the process aborts — and every HIP
    event created during the capture appended to `keep`, so the caller holds
    them for the graph's lifetime (a captured cross-stream wait whose event
    was destroyed after the capture crashed a later replay).  Every event
    record / wait is checked against the nested-join pattern
    (CaptureTopology: raises NestedJoinError instead of reaching a crash in
    hipStreamEndCapture)."""
    import torch.cuda.streams as _streams

    gc.collect()
    was = gc.isenabled()
    gc.disable()
    orig = (torch.cuda.Event, _streams.Event)
    base = orig[0]
    topo = CaptureTopology()
    methods = (base.record, base.wait, _streams.Stream.wait_event)

    def record(ev, stream=None):
        stream = torch.cuda.current_stream() if stream is None else stream
        methods[0](ev, stream)
        topo.recorded(ev, stream)

    def wait(ev, stream=None):
        stream = torch.cuda.current_stream() if stream is None else stream
        if topo.depth == 0:
            topo.waiting(stream, ev)
        methods[1](ev, stream)

    def wait_event(stream, ev):
        topo.waiting(stream, ev)
        topo.depth += 1
        try:
            methods[2](stream, ev)  # torch implements it as ev.wait(stream): checked once, here
        finally:
            topo.depth -= 1

    base.record, base.wait, _streams.Stream.wait_event = record, wait, wait_event
    if keep is not None:

        class _Kept(base):
            def __new__(cls, *a, **k):
                ev = base.__new__(cls, *a, **k)
                keep.append(ev)
                return ev

        torch.cuda.Event = _Kept
        _streams.Event = _Kept
    try:
        yield
    finally:
        torch.cuda.Event, _streams.Event = orig
        base.record, base.wait, _streams.Stream.wait_event = methods
        if was:
            gc.enable()


class Workspace:
    """Grow-only device scratch buffers, one per (device, scope, tag).

    Buffers are reused across calls on the same stream; allocate (warm) them
    before capturing a hipGraph so replays never allocate.  Work issued on a
    concurrent stream runs inside its own `Workspace.scope(name)` so the two
    streams never share a buffer.
    """

    _bufs: Dict[Tuple[int, str], torch.Tensor] = {}
    _scope = ""
    # device addresses each live captured graph may hold (snapshot(owner)), and
    # the buffers a regrowth replaced while such a graph could still address
    # them: kept until no live graph holds their address (the owner's
    # finalizer releases its hold)
    _holds: Dict[int, set] = {}
    _next_hold = 0
    _retired: List[torch.Tensor] = []

    @classmethod
    def _captured(cls) -> set:
        return set().union(*cls._holds.values()) if cls._holds else set()

    @classmethod
    def _release(cls, token: int) -> None:
        cls._holds.pop(token, None)
        live = cls._captured()
        cls._retired = [b for b in cls._retired if b.data_ptr() in live]

    @classmethod
    def get(cls, nbytes: int, device: torch.device, tag: str) -> torch.Tensor:
        key = (device.index if device.index is not None else torch.cuda.current_device(), cls._scope + tag)
        buf = cls._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            if buf is not None and buf.data_ptr() in cls._captured():
                cls._retired.append(buf)  # a live graph may replay into it
            # zeroed once (a fresh sparse workspace carries no recorded error)
            buf = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=device)
            cls._bufs[key] = buf
        return buf

    @classmethod
    def existing(cls, device: torch.device, tag: str, scope: Optional[str] = None) -> Optional[torch.Tensor]:
        """The buffer of (device, scope, tag) if it was ever allocated."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        pre = cls._scope if scope is None else (scope + "/" if scope else "")
        return cls._bufs.get((idx, pre + tag))

    @classmethod
    def all_with_tag(cls, device: torch.device, tag: str) -> List[torch.Tensor]:
        """Every buffer of (device, any scope, tag) allocated so far."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        return [b for (d, k), b in cls._bufs.items() if d == idx and (k == tag or k.endswith("/" + tag))]

    @classmethod
    def clear(cls) -> None:
        """Forget every buffer (those a captured graph may address stay alive)."""
        live = cls._captured()
        cls._retired.extend(b for b in cls._bufs.values() if b.data_ptr() in live)
        cls._bufs.clear()

    @classmethod
    def snapshot(cls, owner=None) -> Dict[Tuple[int, str], int]:
        """{key: device address} of every buffer now allocated.  A captured
        hipGraph holds these addresses: while `owner` (the graph object) is
        alive they are never freed (a regrowth retires the old buffer
        instead); once it is collected its hold is released and retired
        buffers no live graph addresses are freed (owner=None: held for the
        process's lifetime).  Replay the graph only while
        `unchanged(snapshot)` — the host-side readers (sparse_status) look at
        the current buffers."""
        import weakref

        snap = {k: v.data_ptr() for k, v in cls._bufs.items()}
        token = cls._next_hold
        cls._next_hold += 1
        cls._holds[token] = set(snap.values())
        if owner is not None:
            try:
                weakref.finalize(owner, cls._release, token)
            except TypeError:  # not weak-referenceable: held for good
                pass
        return snap

    @classmethod
    def unchanged(cls, snap: Dict[Tuple[int, str], int]) -> bool:
        return all(k in cls._bufs and cls._bufs[k].data_ptr() == p for k, p in snap.items())

    class scope:  # noqa: N801 - context manager named like the operation
        def __init__(self, name: str):
            self.name = name

        def __enter__(self):
            self.prev = Workspace._scope
            Workspace._scope = self.name + "/" if self.name else ""  # "": the root scope
            return self

        def __exit__(self, *exc):
            Workspace._scope = self.prev
            return False


# --------------------------------------------------------------------------
# K2+K3 gather
def _gather_segments(segments, batch: int):
    arr = (GatherSegment * len(segments))()
    for i, (table, ids, off) in enumerate(segments):
        _req(table, f"table[{i}]", torch.float32)
        if not table.is_contiguous():
            raise ValueError(f"table[{i}] must be contiguous")
        if ids is not None:
            _req(ids, f"ids[{i}]", torch.int32)
            if ids.numel() != batch or not ids.is_contiguous():
                raise ValueError(f"ids[{i}] must be a contiguous [{batch}] int32 tensor")
            dim = table.shape[1]
            rows = table.shape[0]
        else:
            if table.numel() != batch:
                raise ValueError(f"numeric column {i} must have {batch} values")
            dim, rows = 1, batch
        arr[i].table = table.data_ptr()
        arr[i].ids = ids.data_ptr() if ids is not None else None
        arr[i].num_rows = rows
        arr[i].dim = dim
        arr[i].col_offset = off
    return arr


def gather_grouped(
    segments: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor], int]],
    batch: int,
    out: torch.Tensor,
) -> torch.Tensor:
    """segments: (table [V,D] or numeric values [B], ids [B] int32 or None, col_offset)."""
    _req(out, "out", torch.float32, 2)
    ld = _row_major(out, "out")
    if len(segments) > _native.MAX_SEGMENTS:
        raise ValueError(f"at most {_native.MAX_SEGMENTS} segments per launch")
    arr = _gather_segments(segments, batch)
    check(lib().tt_gather_grouped(arr, len(segments), batch, out.data_ptr(), ld, _stream()))
    return out


def gather_multi(calls: Sequence[Tuple[Sequence[Tuple[torch.Tensor, Optional[torch.Tensor], int]], torch.Tensor]],
                 batch: int, pack_jobs: Optional[Sequence[Tuple[torch.Tensor, bool, torch.Tensor]]] = None) -> None:
    """Several gather_grouped calls of one batch (e.g. both towers) in one
    launch; pack_jobs (mlp_pack_many's jobs): the weight images packed by the
    same launch (tt_gather_multi_pack)."""
    if sum(len(segs) for segs, _ in calls) > _native.MAX_SEGMENTS:
        raise ValueError(f"at most {_native.MAX_SEGMENTS} segments per launch")
    keep = []
    arr = (_native.GatherCall * len(calls))()
    for i, (segs, out) in enumerate(calls):
        _req(out, f"out[{i}]", torch.float32, 2)
        ld = _row_major(out, f"out[{i}]")
        sa = _gather_segments(segs, batch)
        keep.append(sa)
        arr[i].segs = ctypes.cast(sa, ctypes.c_void_p)
        arr[i].num_segs = len(segs)
        arr[i].out = out.data_ptr()
        arr[i].out_stride = ld
    if pack_jobs:
        check(lib().tt_gather_multi_pack(arr, len(calls), batch, _pack_job_array(pack_jobs), len(pack_jobs),
                                         _stream()))
        return
    check(lib().tt_gather_multi(arr, len(calls), batch, _stream()))


def _sparse_tables(tables: Sequence[dict], batch: int, adam: bool, slots: bool = True):
    arr = (SparseTable * len(tables))()
    for i, t in enumerate(tables):
        table = t["table"]
        _req(table, f"table[{i}]", torch.float32, 2)
        slot0 = t["slot0"] if slots else None
        if not table.is_contiguous():
            raise ValueError(f"table[{i}] must be contiguous")
        if slots:
            _req(slot0, f"slot0[{i}]", torch.float32, 2)
            if not slot0.is_contiguous() or slot0.shape != table.shape:
                raise ValueError(f"table/slot0[{i}] must be contiguous and of equal shape")
        if adam:
            slot1 = t["slot1"]
            _req(slot1, f"slot1[{i}]", torch.float32, 2)
            if not slot1.is_contiguous() or slot1.shape != table.shape:
                raise ValueError(f"slot1[{i}] must be contiguous with the table's shape")
        ids: List[torch.Tensor] = t["ids"]
        offs: List[int] = t["grad_col_offset"]
        if not (1 <= len(ids) <= _native.MAX_SOURCES) or len(ids) != len(offs):
            raise ValueError(f"table[{i}]: 1..{_native.MAX_SOURCES} (ids, col_offset) sources required")
        arr[i].table = table.data_ptr()
        arr[i].slot0 = slot0.data_ptr() if slots else None
        arr[i].slot1 = t["slot1"].data_ptr() if adam else None
        arr[i].num_rows = table.shape[0]
        arr[i].dim = table.shape[1]
        arr[i].num_sources = len(ids)
        for s, (x, o) in enumerate(zip(ids, offs)):
            _req(x, f"ids[{i}][{s}]", torch.int32)
            if x.numel() != batch or not x.is_contiguous():
                raise ValueError(f"ids[{i}][{s}] must be contiguous [{batch}] int32")
            arr[i].ids[s] = x.data_ptr()
            arr[i].grad_col_offset[s] = o
        g = t.get("grad")
        if g is not None:  # per-table gradient buffer (e.g. another tower's input gradient)
            _req(g, f"grad[{i}]", torch.float32, 2)
            if g.shape[0] != batch:
                raise ValueError(f"grad[{i}] must have {batch} rows")
            arr[i].grad = g.data_ptr()
            arr[i].grad_ld = _row_major(g, f"grad[{i}]")
    return arr


def sparse_adagrad(tables: Sequence[dict], batch: int, grad: Optional[torch.Tensor], lr: float,
                   epsilon: float, presorted: bool = False, ws_tag: str = "sparse") -> None:
    """tables: dicts with table, slot0 (accumulator), ids [list], grad_col_offset [list] and an
    optional per-table "grad" [batch, *] that overrides the call's `grad` (which may then be None),
    so one call — one sort — updates the tables of both towers.  presorted: the ids were
    already sorted by sparse_sort(tables, batch) (same tables, stream-ordered before this)."""
    ld = 0
    if grad is not None:
        _req(grad, "grad", torch.float32, 2)
        ld = _row_major(grad, "grad")
    elif any(t.get("grad") is None for t in tables):
        raise ValueError("grad is None but some table has no per-table grad")
    arr = _sparse_tables(tables, batch, adam=False)
    L = lib()
    need = L.tt_sparse_workspace_size(arr, len(tables), batch)
    dev = grad.device if grad is not None else tables[0]["grad"].device
    ws = Workspace.get(need, dev, ws_tag)
    fn = L.tt_sparse_adagrad_sorted if presorted else L.tt_sparse_adagrad
    check(fn(arr, len(tables), batch, grad.data_ptr() if grad is not None else None, ld, lr, epsilon,
             ws.data_ptr(), ws.numel(), _stream()))


def sparse_adagrad_rows(tables: Sequence[Tuple[torch.Tensor, torch.Tensor]], tags: torch.Tensor, rows: torch.Tensor,
                        grad: torch.Tensor, lr: float, epsilon: float) -> None:
    """Adagrad on DISTINCT rows (tt_sparse_adagrad_rows): slot j applies
    grad[j] to row rows[j] of tables[tags[j]] = (table, accumulator);
    invalid tags / rows are skipped.  Each (tag, row) at most once."""
    _req(tags, "tags", torch.int32, 1)
    _req(rows, "rows", torch.int32, 1)
    _req(grad, "grad", torch.float32, 2)
    n = tags.numel()
    if rows.numel() != n or grad.shape[0] < n:
        raise ValueError("tags / rows / grad sizes disagree")
    arr = (SparseTable * len(tables))()
    for i, (t, a) in enumerate(tables):
        _req(t, f"table[{i}]", torch.float32, 2)
        _req(a, f"slot0[{i}]", torch.float32, 2)
        if not (t.is_contiguous() and a.is_contiguous()) or a.shape != t.shape:
            raise ValueError(f"table/slot0[{i}] must be contiguous and of equal shape")
        arr[i].table, arr[i].slot0, arr[i].num_rows, arr[i].dim = t.data_ptr(), a.data_ptr(), t.shape[0], t.shape[1]
    check(lib().tt_sparse_adagrad_rows(arr, len(tables), tags.data_ptr(), rows.data_ptr(), n, grad.data_ptr(),
                                       _row_major(grad, "grad"), lr, epsilon, _stream()))


def sparse_status(device: torch.device, ws_tag: str = "sparse", scope: Optional[str] = None) -> None:
    """Raise TTError if a sparse apply on this workspace recorded an error
    (keys of another call, tt_sparse_status) since the last check.  Synchronises
    the current stream."""
    ws = Workspace.existing(device, ws_tag, scope)
    if ws is None:
        return
    check(lib().tt_sparse_status(ws.data_ptr(), ws.numel(), _stream()))


def sparse_status_all(device: torch.device, ws_tags: Sequence[str]) -> None:
    """sparse_status over every scope's workspace of each tag (all are read
    and cleared; the first recorded error is raised)."""
    err = None
    for tag in ws_tags:
        for ws in Workspace.all_with_tag(device, tag):
            try:
                check(lib().tt_sparse_status(ws.data_ptr(), ws.numel(), _stream()))
            except Exception as e:  # noqa: BLE001 - re-raised below after every workspace is cleared
                err = err or e
    if err is not None:
        raise err


def sparse_sort(tables: Sequence[dict], batch: int, ws_tag: str = "sparse", slots: bool = True) -> None:
    """First stage of sparse_adagrad(..., presorted=True) or
    sparse_scatter_sum(..., presorted=True) (slots=False: tables without
    accumulators): build and sort the lookup keys (reads only the ids; no
    gradient needed), on the current stream."""
    arr = _sparse_tables(tables, batch, adam=False, slots=slots)
    L = lib()
    need = L.tt_sparse_workspace_size(arr, len(tables), batch)
    ws = Workspace.get(need, tables[0]["table"].device, ws_tag)
    check(L.tt_sparse_sort(arr, len(tables), batch, ws.data_ptr(), ws.numel(), _stream()))


def sparse_adam(tables: Sequence[dict], batch: int, grad: torch.Tensor, lr: float, beta1: float, beta2: float,
                epsilon: float, step: int, ws_tag: str = "sparse") -> None:
    _req(grad, "grad", torch.float32, 2)
    ld = _row_major(grad, "grad")
    arr = _sparse_tables(tables, batch, adam=True)
    L = lib()
    need = L.tt_sparse_workspace_size(arr, len(tables), batch)
    ws = Workspace.get(need, grad.device, ws_tag)
    check(L.tt_sparse_adam(arr, len(tables), batch, grad.data_ptr(), ld, lr, beta1, beta2, epsilon, step,
                           ws.data_ptr(), ws.numel(), _stream()))


def sparse_scatter_sum(tables: Sequence[dict], batch: int, grad: torch.Tensor, ws_tag: str = "sparse",
                       presorted: bool = False) -> None:
    """tables: dicts with table (zero-filled dense gradient [rows, dim]), ids
    [list], grad_col_offset [list]; every touched row receives its
    duplicate-summed gradient (tt_sparse_scatter_sum).  presorted: the keys
    were sorted by sparse_sort(tables, batch, ws_tag, slots=False) earlier
    (tt_sparse_scatter_sum_sorted)."""
    _req(grad, "grad", torch.float32, 2)
    ld = _row_major(grad, "grad")
    arr = _sparse_tables(tables, batch, adam=False, slots=False)
    L = lib()
    need = L.tt_sparse_workspace_size(arr, len(tables), batch)
    ws = Workspace.get(need, grad.device, ws_tag)
    fn = L.tt_sparse_scatter_sum_sorted if presorted else L.tt_sparse_scatter_sum
    check(fn(arr, len(tables), batch, grad.data_ptr(), ld, ws.data_ptr(), ws.numel(), _stream()))


def route_requests(lookups: Sequence[Tuple[torch.Tensor, int, int]], world: int, num_tags: int,
                   ordered: bool = False):
    """lookups: (ids [B] int32, table rows, tag).  Returns (send [L*B, 2] int32
    capacity, counts [world] int64, num_requests [1] int32, idx [L, B] int32)
    from tt_route_requests (owner-major deduplicated requests); ordered=True
    appends the route's sorted order (order [L*B], grp_first / grp_last
    [world*num_tags] int32, tt_route_requests_ordered) for sparse_routed."""
    L = len(lookups)
    B = lookups[0][0].numel()
    dev = lookups[0][0].device
    arr = (_native.RouteLookup * L)()
    max_rows = 1
    for i, (ids, rows, tag) in enumerate(lookups):
        _req(ids, f"ids[{i}]", torch.int32, 1)
        if ids.numel() != B or not ids.is_contiguous():
            raise ValueError("route: every lookup needs a contiguous [B] int32 id tensor")
        arr[i].ids = ids.data_ptr()
        arr[i].num_rows = int(rows)
        arr[i].tag = int(tag)
        max_rows = max(max_rows, int(rows))
    send = torch.empty(L * B, 2, dtype=torch.int32, device=dev)
    counts = torch.empty(world, dtype=torch.int64, device=dev)
    nreq = torch.empty(1, dtype=torch.int32, device=dev)
    idx = torch.empty(L, B, dtype=torch.int32, device=dev)
    lib_ = lib()
    ws = Workspace.get(lib_.tt_route_workspace_size(L, B, world, max_rows, num_tags), dev, "route")
    if not ordered:
        check(lib_.tt_route_requests(arr, L, B, world, num_tags, send.data_ptr(), counts.data_ptr(), nreq.data_ptr(),
                                     idx.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        return send, counts, nreq, idx
    order = torch.empty(L * B, dtype=torch.int32, device=dev)
    grp = torch.empty(2, world * num_tags, dtype=torch.int32, device=dev)
    check(lib_.tt_route_requests_ordered(arr, L, B, world, num_tags, send.data_ptr(), counts.data_ptr(),
                                         nreq.data_ptr(), idx.data_ptr(), order.data_ptr(), grp[0].data_ptr(),
                                         grp[1].data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return send, counts, nreq, idx, (order, grp[0], grp[1])


def route_fixed(lookups: Sequence[Tuple[torch.Tensor, int, int]], world: int, num_tags: int, cap: int,
                overflow: Optional[torch.Tensor] = None, ordered: bool = False, owner: bool = False,
                idx_out: Optional[torch.Tensor] = None):
    """The fixed-capacity route in one call (tt_route_fixed; one launch for
    <= 8192 lookups, kRsMax, whose keys fit 32 bits): (send_padded [world*cap, 2], idx_padded [L, B],
    counts [world] int64, (order, grp_first, grp_last) if ordered, and at
    world 1 with owner=True (tags, rows, table_ids [num_tags, cap]) of the
    slots) — equal to route_requests + route_pad (+ route_owner).  idx_out:
    an [L, B] int32 buffer for idx_padded (e.g. a captured step's static one)."""
    L = len(lookups)
    B = lookups[0][0].numel()
    dev = lookups[0][0].device
    arr = (_native.RouteLookup * L)()
    max_rows = 1
    for i, (ids, rows, tag) in enumerate(lookups):
        _req(ids, f"ids[{i}]", torch.int32, 1)
        if ids.numel() != B or not ids.is_contiguous():
            raise ValueError("route: every lookup needs a contiguous [B] int32 id tensor")
        arr[i].ids = ids.data_ptr()
        arr[i].num_rows = int(rows)
        arr[i].tag = int(tag)
        max_rows = max(max_rows, int(rows))
    if owner and world != 1:
        raise ValueError("route_fixed: owner=True is the world-1 shortcut")
    slots = world * cap
    send_p = torch.empty(slots, 2, dtype=torch.int32, device=dev)
    if idx_out is not None:
        _req(idx_out, "idx_out", torch.int32, 2)
        if tuple(idx_out.shape) != (L, B) or not idx_out.is_contiguous():
            raise ValueError(f"route_fixed: idx_out must be a contiguous [{L}, {B}] int32 buffer")
    idx_p = idx_out if idx_out is not None else torch.empty(L, B, dtype=torch.int32, device=dev)
    counts = torch.empty(world, dtype=torch.int64, device=dev)
    if overflow is not None:
        _req(overflow, "overflow", torch.int32, 1)
    order = grp = own = None
    if ordered:
        order = torch.empty(L * B, dtype=torch.int32, device=dev)
        grp = torch.empty(2, world * num_tags, dtype=torch.int32, device=dev)
    if owner:
        own = (torch.empty(slots, dtype=torch.int32, device=dev), torch.empty(slots, dtype=torch.int32, device=dev),
               torch.empty(num_tags, slots, dtype=torch.int32, device=dev))
    lib_ = lib()
    ws = Workspace.get(lib_.tt_route_fixed_workspace_size(L, B, world, max_rows, num_tags), dev, "route")
    check(lib_.tt_route_fixed(arr, L, B, world, num_tags, cap, send_p.data_ptr(), idx_p.data_ptr(), counts.data_ptr(),
                              _ptr(overflow), _ptr(order), _ptr(grp[0] if grp is not None else None),
                              _ptr(grp[1] if grp is not None else None), *(_ptr(t) for t in (own or (None,) * 3)),
                              ws.data_ptr(), ws.numel(), _stream()))
    return send_p, idx_p, counts, (order, grp[0], grp[1]) if ordered else None, own


def sparse_routed(tables: Sequence[dict], batch: int, grad: Optional[torch.Tensor], route: dict, op: str,
                  lr: float = 0.0, epsilon: float = 0.0, ws_tag: str = "sparse_routed") -> None:
    """Per-request sums (op "sum", tt_sparse_scatter_sum semantics) or the
    Adagrad update (op "adagrad", tables need slot0) of routed lookups, keyed
    by the route's own sort (tt_sparse_routed: no second sort).  tables: as
    for sparse_scatter_sum / sparse_adagrad (ids = each source lookup's slots).
    route: order, grp_first, grp_last (route_requests(..., ordered=True)),
    slot ([L, B] slots of every routed lookup), slot_row (optional [world*cap]
    keys per slot), cap, world, num_tags and per routed lookup l its
    lookup_tag / lookup_table / lookup_source."""
    ld = 0
    if grad is not None:
        _req(grad, "grad", torch.float32, 2)
        ld = _row_major(grad, "grad")
    elif any(t.get("grad") is None for t in tables):
        raise ValueError("grad is None but some table has no per-table grad")
    if op not in ("sum", "adagrad"):
        raise ValueError(f"sparse_routed: op must be 'sum' or 'adagrad', got {op!r}")
    arr = _sparse_tables(tables, batch, adam=False, slots=op == "adagrad")
    rs = _native.RouteSorted()
    for name in ("order", "grp_first", "grp_last", "slot"):
        t = route[name]
        _req(t, name, torch.int32)
        if not t.is_contiguous():
            raise ValueError(f"sparse_routed: {name} must be contiguous")
        setattr(rs, name, t.data_ptr())
    rs.slot_row = _ptr(route.get("slot_row"))
    rs.cap, rs.world, rs.num_tags = int(route["cap"]), int(route["world"]), int(route["num_tags"])
    L = len(route["lookup_tag"])
    if L > _native.ROUTE_MAX_LOOKUPS:
        raise ValueError(f"sparse_routed: at most {_native.ROUTE_MAX_LOOKUPS} routed lookups, got {L}")
    rs.num_lookups = L
    for i in range(L):
        rs.lookup_tag[i] = int(route["lookup_tag"][i])
        rs.lookup_table[i] = int(route["lookup_table"][i])
        rs.lookup_source[i] = int(route["lookup_source"][i])
    lib_ = lib()
    need = lib_.tt_sparse_workspace_size(arr, len(tables), batch)
    dev = grad.device if grad is not None else tables[0]["grad"].device
    ws = Workspace.get(need, dev, ws_tag)
    check(lib_.tt_sparse_routed(arr, len(tables), batch, grad.data_ptr() if grad is not None else None, ld,
                                ctypes.byref(rs), 1 if op == "adagrad" else 0, lr, epsilon, ws.data_ptr(), ws.numel(),
                                _stream()))


def route_pad(send: torch.Tensor, counts: torch.Tensor, idx: torch.Tensor, world: int, cap: int,
              overflow: Optional[torch.Tensor] = None):
    """The compact requests of route_requests in `cap` fixed slots per owner
    (tt_route_pad): (send_padded [world*cap, 2], idx_padded like idx).  No
    host sync; `overflow` (int32 [1], optional) counts dropped requests."""
    _req(send, "send", torch.int32, 2)
    _req(counts, "counts", torch.int64, 1)
    _req(idx, "idx", torch.int32)
    if counts.numel() != world or not idx.is_contiguous():
        raise ValueError("route_pad: counts must be [world], idx contiguous")
    send_p = torch.empty(world * cap, 2, dtype=torch.int32, device=send.device)
    idx_p = torch.empty_like(idx)
    if overflow is not None:
        _req(overflow, "overflow", torch.int32, 1)
    check(lib().tt_route_pad(send.data_ptr(), counts.data_ptr(), idx.data_ptr(), idx.numel(), world, cap,
                             send_p.data_ptr(), idx_p.data_ptr(), _ptr(overflow), _stream()))
    return send_p, idx_p


def route_owner(recv: torch.Tensor, world: int, num_tags: int):
    """recv [n, 2] int32 requests received by this owner -> (tags [n], local rows
    [n], table_ids [num_tags, n]) from tt_route_owner."""
    _req(recv, "recv", torch.int32, 2)
    n = recv.shape[0]
    tags = torch.empty(n, dtype=torch.int32, device=recv.device)
    rows = torch.empty(n, dtype=torch.int32, device=recv.device)
    tids = torch.empty(num_tags, n, dtype=torch.int32, device=recv.device)
    check(lib().tt_route_owner(recv.contiguous().data_ptr(), n, world, num_tags, tags.data_ptr(), rows.data_ptr(),
                               tids.data_ptr(), _stream()))
    return tags, rows, tids


def gather_tagged(tables: Sequence[torch.Tensor], tags: torch.Tensor, rows: torch.Tensor,
                  out: torch.Tensor) -> torch.Tensor:
    """out[j] = tables[tags[j]][rows[j]] (zero row when invalid); tables share dim."""
    _req(tags, "tags", torch.int32, 1)
    _req(rows, "rows", torch.int32, 1)
    _req(out, "out", torch.float32, 2)
    ld = _row_major(out, "out")
    dim = tables[0].shape[1]
    arr = (_native.RowTable * len(tables))()
    for i, t in enumerate(tables):
        _req(t, f"tables[{i}]", torch.float32, 2)
        if t.shape[1] != dim or not t.is_contiguous():
            raise ValueError("tables must be contiguous and share one dim")
        arr[i].table = t.data_ptr()
        arr[i].num_rows = t.shape[0]
    n = tags.numel()
    if rows.numel() != n or out.shape[0] < n or out.shape[1] < dim:
        raise ValueError("tags/rows/out sizes disagree")
    check(lib().tt_gather_tagged(arr, len(tables), dim, tags.data_ptr(), rows.data_ptr(), n, out.data_ptr(), ld,
                                 _stream()))
    return out


def dedup_sum(ids: torch.Tensor, grad: torch.Tensor, num_rows: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Distinct ids (ascending) and per-id gradient sums (K8)."""
    _req(ids, "ids", torch.int32, 1)
    _req(grad, "grad", torch.float32, 2)
    ld = _row_major(grad, "grad")
    n, dim = ids.numel(), grad.shape[1]
    if grad.shape[0] != n:
        raise ValueError("grad must have one row per id")
    L = lib()
    ws = Workspace.get(L.tt_dedup_workspace_size(n, dim), grad.device, "dedup")
    uniq = torch.empty(n, dtype=torch.int32, device=grad.device)
    summed = torch.empty(n, dim, dtype=torch.float32, device=grad.device)
    count = torch.empty(1, dtype=torch.int32, device=grad.device)
    check(L.tt_dedup_sum(ids.data_ptr(), n, num_rows, grad.data_ptr(), ld, dim, uniq.data_ptr(), summed.data_ptr(),
                         count.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    u = int(count.item())
    return uniq[:u], summed[:u]


def loss_sum(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """0-d tensor scale * x.sum() (tt_sum: one deterministic launch)."""
    _req(x, "x", torch.float32)
    if not x.is_contiguous():
        raise ValueError("x must be contiguous")
    out = torch.empty((), dtype=torch.float32, device=x.device)
    check(lib().tt_sum(x.data_ptr(), x.numel(), float(scale), out.data_ptr(), _stream()))
    return out


def dense_adagrad(param: torch.Tensor, accum: torch.Tensor, grad: torch.Tensor, lr: float, epsilon: float) -> None:
    for t, n in ((param, "param"), (accum, "accum"), (grad, "grad")):
        _req(t, n, torch.float32)
        if not t.is_contiguous() or t.numel() != param.numel():
            raise ValueError(f"{n} must be contiguous with param's numel")
    check(lib().tt_dense_adagrad(param.data_ptr(), accum.data_ptr(), grad.data_ptr(), param.numel(), lr, epsilon,
                                 _stream()))


def dense_adagrad_many(jobs: Sequence[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]], lr: float,
                       epsilon: float) -> None:
    """dense_adagrad on up to 8 (param, accum, grad) buffers in one launch
    (tt_dense_adagrad_many; bit-identical to one call each)."""
    arr = (_native.DenseJob * len(jobs))()
    for i, (p, a, g) in enumerate(jobs):
        for name, t in (("param", p), ("accum", a), ("grad", g)):
            _req(t, f"{name}[{i}]", torch.float32)
            if not t.is_contiguous() or t.numel() != p.numel():
                raise ValueError(f"dense_adagrad_many: {name}[{i}] must be contiguous with param's size")
        arr[i].param, arr[i].accum, arr[i].grad, arr[i].n = p.data_ptr(), a.data_ptr(), g.data_ptr(), p.numel()
    check(lib().tt_dense_adagrad_many(arr, len(jobs), lr, epsilon, _stream()))


def dense_adam(param, m, v, grad, lr, beta1, beta2, epsilon, step) -> None:
    for t, n in ((param, "param"), (m, "m"), (v, "v"), (grad, "grad")):
        _req(t, n, torch.float32)
        if not t.is_contiguous() or t.numel() != param.numel():
            raise ValueError(f"{n} must be contiguous with param's numel")
    check(lib().tt_dense_adam(param.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), param.numel(), lr,
                              beta1, beta2, epsilon, step, _stream()))


# -- Adam with the step count on the device (tt_adam_clock) -------------------
def adam_coef_len(beta1: float, beta2: float) -> int:
    """tt_adam_coef_len: the first step from which both Adam coefficients equal
    the learning rate in fp32 (0: a beta outside [0, 1), or more than 2^22 steps)."""
    return int(lib().tt_adam_coef_len(beta1, beta2))


def adam_coef_tables(lr: float, beta1: float, beta2: float, length: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """tt_adam_coef_fill: host float32 tensors (alpha [length], lr_t [length]), entry t-1 for step t."""
    alpha = torch.empty(max(length, 0), dtype=torch.float32)
    lr_t = torch.empty(max(length, 0), dtype=torch.float32)
    check(lib().tt_adam_coef_fill(lr, beta1, beta2, length, alpha.data_ptr(), lr_t.data_ptr()))
    return alpha, lr_t


def _req_clock(clock: torch.Tensor) -> None:
    _req(clock, "clock", torch.int64, 1)
    if clock.numel() != 2 or not clock.is_contiguous():
        raise ValueError("clock must be a contiguous int64 [2] tensor (the 16-byte tt_adam_clock)")


def adam_clock_advance(clock: torch.Tensor, alpha_tab: torch.Tensor, lr_t_tab: torch.Tensor) -> None:
    """tt_adam_clock_advance on the current stream: clock (int64 [2]: the step
    word, then the float32 pair) moves one step along the device tables."""
    _req_clock(clock)
    for t, n in ((alpha_tab, "alpha_tab"), (lr_t_tab, "lr_t_tab")):
        _req(t, n, torch.float32, 1)
        if not t.is_contiguous() or t.numel() != alpha_tab.numel() or t.numel() < 1:
            raise ValueError(f"{n} must be a contiguous, non-empty table of alpha_tab's length")
    check(lib().tt_adam_clock_advance(clock.data_ptr(), alpha_tab.data_ptr(), lr_t_tab.data_ptr(),
                                      alpha_tab.numel(), _stream()))


def dense_adam_many_dev(jobs: Sequence[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]], beta1: float,
                        beta2: float, epsilon: float, clock: torch.Tensor) -> None:
    """dense_adam on up to 8 (param, m, v, grad) buffers in one launch, the
    step's coefficient read from `clock` on the device (tt_dense_adam_many_dev)."""
    _req_clock(clock)
    arr = (_native.DenseAdamJob * len(jobs))()
    for i, (p, m, v, g) in enumerate(jobs):
        for name, t in (("param", p), ("m", m), ("v", v), ("grad", g)):
            _req(t, f"{name}[{i}]", torch.float32)
            if not t.is_contiguous() or t.numel() != p.numel():
                raise ValueError(f"dense_adam_many_dev: {name}[{i}] must be contiguous with param's size")
        arr[i].param, arr[i].m, arr[i].v, arr[i].grad, arr[i].n = (p.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                                   g.data_ptr(), p.numel())
    check(lib().tt_dense_adam_many_dev(arr, len(jobs), beta1, beta2, epsilon, clock.data_ptr(), _stream()))


def sparse_adam_dev(tables: Sequence[dict], batch: int, grad: Optional[torch.Tensor], beta1: float, beta2: float,
                    epsilon: float, clock: torch.Tensor, ws_tag: str = "sparse") -> None:
    """sparse_adam with the step's coefficient read from `clock` on the device
    and the whole-table stages of all tables in one launch each
    (tt_sparse_adam_dev).  grad may be None when every table brings its own
    "grad" (one call for the tables of both towers, as sparse_adagrad)."""
    _req_clock(clock)
    ld = 0
    if grad is not None:
        _req(grad, "grad", torch.float32, 2)
        ld = _row_major(grad, "grad")
    elif any(t.get("grad") is None for t in tables):
        raise ValueError("grad is None but some table has no per-table grad")
    arr = _sparse_tables(tables, batch, adam=True)
    L = lib()
    need = L.tt_sparse_workspace_size(arr, len(tables), batch)
    ws = Workspace.get(need, clock.device, ws_tag)
    check(L.tt_sparse_adam_dev(arr, len(tables), batch, grad.data_ptr() if grad is not None else None, ld, beta1,
                               beta2, epsilon, clock.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))


# --------------------------------------------------------------------------
# K5+K6+K7 fused in-batch softmax cross-entropy
# --------------------------------------------------------------------------
# Measurement hook: time ONE kernel of a multi-launch entry point (tt_probe_arm)
PROBE_INBATCH_ROWS, PROBE_INBATCH_COLS, PROBE_INDEX_SCREEN, PROBE_INDEX_FINALIZE = range(4)


def probe_arm(kernel: int, start: "torch.cuda.Event", stop: "torch.cuda.Event") -> None:
    """The next launch of `kernel` on this thread records `start` / `stop`
    (timing-enabled torch.cuda.Events) on its own launch stream."""
    for ev in (start, stop):
        if not ev.cuda_event:  # torch creates the HIP event on first record
            ev.record()
    check(lib().tt_probe_arm(kernel, start.cuda_event, stop.cuda_event))


def probe_arm_repeat(kernel: int, start: "torch.cuda.Event", stop: "torch.cuda.Event", reps: int) -> None:
    """As probe_arm, and the armed in-batch pass is launched `reps` times back
    to back between the events (tt_probe_arm_repeat)."""
    for ev in (start, stop):
        if not ev.cuda_event:
            ev.record()
    check(lib().tt_probe_arm_repeat(kernel, start.cuda_event, stop.cuda_event, int(reps)))


def _opt_ptr(t: Optional[torch.Tensor], name: str, n: int) -> Optional[int]:
    if t is None:
        return None
    _req(t, name, torch.float32, 1)
    if t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous [{n}] float32 tensor")
    return t.data_ptr()


def _ids_ptr(t: torch.Tensor, name: str, like: torch.Tensor) -> int:
    """Candidate ids of the accidental-hit entries: a contiguous int32 vector,
    one id per row of `like`, on its device (checked before the operands, so
    a bad id vector is reported as such wherever the operands live)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != torch.int32:
        raise TypeError(f"{name} must be torch.int32, got {t.dtype}")
    n = like.shape[0]
    if t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous [{n}] int32 tensor, got shape {tuple(t.shape)}")
    if t.device != like.device:
        raise ValueError(f"{name} must live on the operands' device {like.device} (got {t.device})")
    return t.data_ptr()


def _ids_pair(row_ids, col_ids, rows: torch.Tensor, cols: torch.Tensor):
    """(row_ids pointer, col_ids pointer), or None when neither is given."""
    if (row_ids is None) != (col_ids is None):
        raise ValueError("row_ids and col_ids go together (both or neither)")
    if row_ids is None:
        return None
    return _ids_ptr(row_ids, "row_ids", rows), _ids_ptr(col_ids, "col_ids", cols)


def _hard_k(k) -> int:
    """num_hard_negatives as the library takes it: a positive int."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"the number of hard negatives must be a positive int, got {k!r}")
    return k


def _inbatch_operands(q: torch.Tensor, c: torch.Tensor, shapes: Optional[str] = "dim"):
    """The in-batch entries' operand checks: (ldq, ldc, R, C, E) of q [R, E]
    and c [C, E].  shapes: the agreement asked of them — "dim" (one embedding
    size), "square" (C = R), "mixed" (C >= R) or None (left to the library)."""
    _req(q, "q", torch.float32, 2)
    _req(c, "c", torch.float32, 2)
    ldq, ldc = _row_major(q, "q"), _row_major(c, "c")
    R, E = q.shape
    C = c.shape[0]
    if shapes == "dim" and c.shape[1] != E:
        raise ValueError("q and c must share the embedding size")
    if shapes == "square" and tuple(c.shape) != (R, E):
        raise ValueError("q and c must both be [B, E]")
    if shapes == "mixed" and (c.shape[1] != E or C < R):
        raise ValueError(f"c must be [B + M, E] with M >= 0 for q [B, E], got {tuple(c.shape)} for {tuple(q.shape)}")
    return ldq, ldc, R, C, E


def _inbatch_variant(L, R: int, C: int, E: int, device: torch.device, x3: bool, hits, hard: bool = False,
                     mixed: bool = False):
    """What the options change in a rows / cols / threshold call: (the entry's
    suffix, its workspace, the arguments (row_ids, col_ids, x3) after
    pos_offset — none for the plain and _x3 entries, which have no such
    parameters).  hits: _ids_pair's result."""
    kind = "mixed" if mixed else "hard" if hard else "hits" if hits is not None else None
    if kind is None:
        size = (L.tt_inbatch_x3_workspace_size if x3 else L.tt_inbatch_workspace_size)(R, C, E)
        suffix, tag, mid = "_x3" if x3 else "", "inbatch", ()
    else:
        size = getattr(L, f"tt_inbatch_{kind}_workspace_size")(R, C, E, int(x3))
        suffix, tag, mid = "_" + kind, "inbatch_" + kind, (*(hits or (None, None)), int(x3))
    return suffix, Workspace.get(size, device, tag + ("_x3" if x3 else "")), mid


def _empty(device: torch.device, *shape: int) -> torch.Tensor:
    return torch.empty(shape, dtype=torch.float32, device=device)


def inbatch_hard_threshold(q: torch.Tensor, c: torch.Tensor, logq: Optional[torch.Tensor], k: int,
                           pos_offset: int = 0, x3: bool = False, row_ids: Optional[torch.Tensor] = None,
                           col_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Hard-negative mining, the selection (tt_inbatch_hard_threshold): thr [R],
    each row's threshold between its k-th and (k+1)-th largest negative score
    S' = q_i . c_j - logq[j] in the arithmetic the passes use (x3, hits by
    row_ids / col_ids as in inbatch_rows); -inf where the row has at most k
    negatives.  Passed as thr= to inbatch_rows / inbatch_cols, only negatives
    with S' >= thr keep their weight; negatives that tie the k-th value are
    all kept (include/tt.h)."""
    k = _hard_k(k)
    hits = _ids_pair(row_ids, col_ids, q, c)
    ldq, ldc, R, C, E = _inbatch_operands(q, c)
    L = lib()
    _, ws, mid = _inbatch_variant(L, R, C, E, q.device, x3, hits, hard=True)
    thr = _empty(q.device, R)
    check(L.tt_inbatch_hard_threshold(q.data_ptr(), ldq, R, c.data_ptr(), ldc, C, E, _opt_ptr(logq, "logq", C),
                                      pos_offset, *mid, k, thr.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return thr


def inbatch_rows(q: torch.Tensor, c: torch.Tensor, logq: Optional[torch.Tensor], pos_offset: int = 0,
                 want_dq: bool = True, x3: bool = False, row_ids: Optional[torch.Tensor] = None,
                 col_ids: Optional[torch.Tensor] = None, thr: Optional[torch.Tensor] = None):
    """Row pass: (lse [R], row_loss [R], dq [R,E] or None).  x3: fp32-faithful
    products (tt_inbatch_xent_rows_x3, as inbatch_fused(x3=True)).
    row_ids [R], col_ids [C] (int32, both or neither): accidental hits
    removed (tt_inbatch_xent_rows_hits) — a column j other than row i's
    positive with col_ids[j] == row_ids[i] is no negative of row i.  Ids are
    compared for equality only, so all out-of-vocabulary rows (id 0) count
    as one candidate.  thr [R] (inbatch_hard_threshold's, same operands, ids
    and x3): hard-negative mining (tt_inbatch_xent_rows_hard) — a negative
    with S' below its row's threshold has weight 0."""
    hits = _ids_pair(row_ids, col_ids, q, c)
    ldq, ldc, R, C, E = _inbatch_operands(q, c)
    L = lib()
    lse, row_loss = _empty(q.device, R), _empty(q.device, R)
    dq = _empty(q.device, R, E) if want_dq else None
    suffix, ws, mid = _inbatch_variant(L, R, C, E, q.device, x3, hits, hard=thr is not None)
    head = (q.data_ptr(), ldq, R, c.data_ptr(), ldc, C, E, _opt_ptr(logq, "logq", C), pos_offset)
    if thr is not None:
        mid += (_opt_ptr(thr, "thr", R),)
    check(getattr(L, "tt_inbatch_xent_rows" + suffix)(
        *head, *mid, lse.data_ptr(), row_loss.data_ptr(), dq.data_ptr() if dq is not None else None, ws.data_ptr(),
        ws.numel(), _stream()))
    return lse, row_loss, dq


def inbatch_cols(q: torch.Tensor, lse: torch.Tensor, c: torch.Tensor, logq: Optional[torch.Tensor],
                 pos_offset: int = 0, row_loss: Optional[torch.Tensor] = None, x3: bool = False,
                 row_ids: Optional[torch.Tensor] = None, col_ids: Optional[torch.Tensor] = None,
                 thr: Optional[torch.Tensor] = None, mixed: bool = False) -> torch.Tensor:
    """Column pass: dc [C,E] from every row's q [R,E], lse [R] and (optional,
    for the exact 1 - P_pos of confident rows) row_loss [R].  x3: fp32-faithful
    products (tt_inbatch_xent_cols_x3).  row_ids [R], col_ids [C] (int32, both
    or neither): accidental hits removed as in inbatch_rows, whose lse and
    row_loss must come from the same ids (tt_inbatch_xent_cols_hits).
    thr [R]: every row's hard-negative threshold, the one its lse came from
    (tt_inbatch_xent_cols_hard).  mixed: columns whose positive row j +
    pos_offset falls outside [0, R) are extra negatives of every row with no
    positive term (tt_inbatch_xent_cols_mixed; ids and thr as above, or
    none)."""
    hits = _ids_pair(row_ids, col_ids, q, c)
    ldq, ldc, R, C, E = _inbatch_operands(q, c, shapes=None)  # (c's width is the library's to check, as ldc)
    L = lib()
    dc = _empty(q.device, C, E)
    suffix, ws, mid = _inbatch_variant(L, R, C, E, q.device, x3, hits, hard=thr is not None, mixed=mixed)
    head = (q.data_ptr(), ldq, R, _opt_ptr(lse, "lse", R), _opt_ptr(row_loss, "row_loss", R), c.data_ptr(), ldc, C, E,
            _opt_ptr(logq, "logq", C), pos_offset)
    if mixed or thr is not None:  # (the mixed entry takes thr or NULL)
        mid += (_opt_ptr(thr, "thr", R),)
    check(getattr(L, "tt_inbatch_xent_cols" + suffix)(*head, *mid, dc.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      _stream()))
    return dc


def inbatch_weight_rows(w: torch.Tensor, lse: torch.Tensor, row_loss: torch.Tensor,
                        dq: Optional[torch.Tensor] = None):
    """Per-example sample weights folded in between inbatch_rows and
    inbatch_cols (tt_inbatch_weight_rows, one launch): (lse_w [R],
    row_loss_w [R], wloss [R]).  w [R]: the normalised weights in [0, 1];
    lse, row_loss: inbatch_rows' outputs.  inbatch_cols(q, lse_w, ...,
    row_loss=row_loss_w) then returns the weighted loss's dc, and wloss holds
    the weighted loss terms w_i * row_loss_i.  dq [R, E] (inbatch_rows'), if
    given, is scaled by w IN PLACE (a weight-0 row stored as zeros, a
    weight-1 row not touched).  A weight outside [0, 1] gives NaN in its row.
    The three outputs are views of a Workspace buffer (a captured step keeps
    their addresses): the next call in the same scope overwrites them."""
    _req(w, "w", torch.float32, 1)
    n = w.numel()
    pw, pl, pr = _opt_ptr(w, "w", n), _opt_ptr(lse, "lse", n), _opt_ptr(row_loss, "row_loss", n)
    lddq, dim = 0, 0
    if dq is not None:
        _req(dq, "dq", torch.float32, 2)
        if dq.shape[0] != n:
            raise ValueError(f"dq must have one row per weight ({n}), got shape {tuple(dq.shape)}")
        lddq, dim = _row_major(dq, "dq"), dq.shape[1]
    seg = (n + 63) // 64 * 64  # each output 256-B aligned
    out = Workspace.get(3 * seg * 4, w.device, "inbatch_weight")[:3 * seg * 4].view(torch.float32)
    lse_w, row_loss_w, wloss = (out[i * seg:i * seg + n] for i in range(3))
    check(lib().tt_inbatch_weight_rows(pw, pl, pr, n, lse_w.data_ptr(), row_loss_w.data_ptr(), wloss.data_ptr(),
                                       dq.data_ptr() if dq is not None else None, lddq, dim, _stream()))
    return lse_w, row_loss_w, wloss


def inbatch_fused_workspace(B: int, E: int, device: torch.device) -> torch.Tensor:
    """The fused entry's workspace in the current scope (fetch it before
    forking per-tower streams so inbatch_prep on either stream and the
    fused call share it)."""
    return Workspace.get(lib().tt_inbatch_fused_workspace_size(B, E), device, "inbatch_fused")


def inbatch_prep(x: torch.Tensor, operand: int, logq: Optional[torch.Tensor], ws: torch.Tensor) -> None:
    """bf16 preparation of one operand of inbatch_fused into `ws` on the
    current stream: operand 0 = q, 1 = c (+ the logQ bias vectors)."""
    _req(x, "x", torch.float32, 2)
    ld = _row_major(x, "x")
    B, E = x.shape
    check(lib().tt_inbatch_prep(x.data_ptr(), ld, B, E, int(operand), _opt_ptr(logq, "logq", B) if operand else None,
                                ws.data_ptr(), ws.numel(), _stream()))


def inbatch_fused(q: torch.Tensor, c: torch.Tensor, logq: Optional[torch.Tensor], ws: Optional[torch.Tensor] = None,
                  prepped: bool = False, loss_scale: Optional[float] = None, x3: bool = False,
                  ids: Optional[torch.Tensor] = None, hard_k: Optional[int] = None):
    """Single-device loss + gradients (both passes, shared bf16 prep):
    (lse [B], row_loss [B], dq [B,E], dc [B,E]).  prepped: both operands were
    already prepared into `ws` by inbatch_prep (ordered before this call).
    loss_scale: also return the loss loss_scale * sum(row_loss) (a 0-d
    tensor, computed inside the last launch, equal to loss_sum's).
    x3: fp32-faithful products (tt_inbatch_softmax_xent_x3: S and P.V as
    bf16x3 products, ~3x the passes' time; not with prepped).
    ids [B] (int32): accidental hits removed (tt_inbatch_softmax_xent_hits) —
    a column j != i with ids[j] == ids[i] is no negative of row i; equality
    only, so all out-of-vocabulary rows (id 0) count as one candidate.  This
    departs from the reference's loss; not with prepped.
    hard_k: hard-negative mining (tt_inbatch_softmax_xent_hard: one
    preparation, then selection, rows, cols) — only each row's hard_k
    largest-scoring negatives (and those tying the last) keep their weight;
    with or without ids, either arithmetic, not with prepped.  The row
    thresholds come back as one more value after dc: (lse, row_loss, dq, dc,
    thr[, loss])."""
    if hard_k is not None:
        hard_k = _hard_k(hard_k)
        if prepped:
            raise ValueError("hard_k: the hard-negative entry prepares its operands itself (prepped=False)")
    if ids is not None:
        if prepped:
            raise ValueError("ids: the accidental-hit entry prepares its operands itself (prepped=False)")
        idp = _ids_ptr(ids, "ids", q)
    ldq, ldc, B, _, E = _inbatch_operands(q, c, shapes="square")
    if prepped and ws is None:
        raise ValueError("prepped=True needs the workspace the operands were prepared into")
    L = lib()
    kind = "hard" if hard_k is not None else "hits" if ids is not None else "x3" if x3 else None
    if kind == "x3":
        if prepped:
            raise ValueError("x3: the fp32-faithful entry prepares its operands itself (prepped=False)")
        ws = Workspace.get(L.tt_inbatch_fused_x3_workspace_size(B, E), q.device, "inbatch_fused_x3")
    elif kind is not None:  # (each with a workspace of its own, whatever ws is)
        ws = Workspace.get(getattr(L, f"tt_inbatch_fused_{kind}_workspace_size")(B, E, int(x3)), q.device,
                           f"inbatch_fused_{kind}" + ("_x3" if x3 else ""))
    elif ws is None:
        ws = inbatch_fused_workspace(B, E, q.device)
    lse, row_loss, dq, dc = _empty(q.device, B), _empty(q.device, B), _empty(q.device, B, E), _empty(q.device, B, E)
    thr = _empty(q.device, B) if hard_k is not None else None
    loss = _empty(q.device) if loss_scale is not None else None
    # (loss_scale, loss): after the outputs of every entry but the plain and the prepped one
    sl = (float(loss_scale if loss_scale is not None else 1.0), loss.data_ptr() if loss is not None else None)
    # the entry, its arguments between logq and the outputs, and between the outputs and the workspace
    fn, mid, end = {
        "hard": (L.tt_inbatch_softmax_xent_hard, (idp if ids is not None else None, int(x3), hard_k),
                 (thr.data_ptr() if thr is not None else None, *sl)),
        "hits": (L.tt_inbatch_softmax_xent_hits, (idp if ids is not None else None, int(x3)), sl),
        "x3": (L.tt_inbatch_softmax_xent_x3, (), sl),
        "loss": (L.tt_inbatch_softmax_xent_loss, (), (*sl, int(prepped))),
        "prepped": (L.tt_inbatch_softmax_xent_prepped, (), ()),
        "plain": (L.tt_inbatch_softmax_xent, (), ()),
    }[kind or ("loss" if loss is not None else "prepped" if prepped else "plain")]
    check(fn(q.data_ptr(), ldq, c.data_ptr(), ldc, B, E, _opt_ptr(logq, "logq", B), *mid, lse.data_ptr(),
             row_loss.data_ptr(), dq.data_ptr(), dc.data_ptr(), *end, ws.data_ptr(), ws.numel(), _stream()))
    return (lse, row_loss, dq, dc) + ((thr,) if thr is not None else ()) + ((loss,) if loss is not None else ())


def inbatch_fused_mixed(q: torch.Tensor, c: torch.Tensor, logq: Optional[torch.Tensor],
                        loss_scale: Optional[float] = None, x3: bool = False, ids: Optional[torch.Tensor] = None,
                        hard_k: Optional[int] = None):
    """inbatch_fused with extra negatives (tt_inbatch_softmax_xent_mixed):
    q [B, E] against c [B + M, E], row i's positive column i, columns past B
    negatives of every row (mixed negative sampling).  logq and ids have
    B + M entries.  Returns (lse [B], row_loss [B], dq [B, E], dc [B + M, E]
    [, thr [B] with hard_k][, loss with loss_scale]); M = 0 is inbatch_fused."""
    if hard_k is not None:
        hard_k = _hard_k(hard_k)
    idp = _ids_ptr(ids, "ids", c) if ids is not None else None
    ldq, ldc, B, C, E = _inbatch_operands(q, c, shapes="mixed")
    M = C - B
    L = lib()
    ws = Workspace.get(L.tt_inbatch_fused_mixed_workspace_size(B, M, E, int(x3)), q.device,
                       "inbatch_fused_mixed_x3" if x3 else "inbatch_fused_mixed")
    lse, row_loss, dq, dc = _empty(q.device, B), _empty(q.device, B), _empty(q.device, B, E), _empty(q.device, C, E)
    thr = _empty(q.device, B) if hard_k is not None else None
    loss = _empty(q.device) if loss_scale is not None else None
    check(L.tt_inbatch_softmax_xent_mixed(q.data_ptr(), ldq, B, c.data_ptr(), ldc, M, E,
                                          _opt_ptr(logq, "logq", B + M), idp, int(x3), hard_k or 0, lse.data_ptr(),
                                          row_loss.data_ptr(), dq.data_ptr(), dc.data_ptr(),
                                          thr.data_ptr() if thr is not None else None,
                                          float(loss_scale if loss_scale is not None else 1.0),
                                          loss.data_ptr() if loss is not None else None, ws.data_ptr(), ws.numel(),
                                          _stream()))
    return (lse, row_loss, dq, dc) + ((thr,) if thr is not None else ()) + ((loss,) if loss is not None else ())


# --------------------------------------------------------------------------
# K11+K12 brute-force index
def bruteforce_build(cand: torch.Tensor) -> torch.Tensor:
    _req(cand, "cand", torch.float32, 2)
    ld = _row_major(cand, "cand")
    n, d = cand.shape
    L = lib()
    nbytes = L.tt_bruteforce_index_bytes(n, d)
    if nbytes == 0:
        raise ValueError(f"unsupported index shape {tuple(cand.shape)}")
    index = torch.empty(nbytes, dtype=torch.uint8, device=cand.device)
    check(L.tt_bruteforce_build(cand.data_ptr(), ld, n, d, index.data_ptr(), nbytes, _stream()))
    return index


def bruteforce_search(index: torch.Tensor, cand: torch.Tensor, queries: torch.Tensor, k: int,
                      index_offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    _req(index, "index", torch.uint8, 1)
    _req(cand, "cand", torch.float32, 2)
    _req(queries, "queries", torch.float32, 2)
    ldc, ldq = _row_major(cand, "cand"), _row_major(queries, "queries")
    n, d = cand.shape
    nq = queries.shape[0]
    if queries.shape[1] != d:
        raise ValueError("queries and candidates must share the embedding size")
    if k > n:
        raise ValueError(f"k={k} exceeds the number of candidates {n}")
    L = lib()
    ws = Workspace.get(L.tt_bruteforce_workspace_size(max(nq, 1), n, d, k), queries.device, "bruteforce")
    out_s = torch.empty(nq, k, dtype=torch.float32, device=queries.device)
    out_i = torch.empty(nq, k, dtype=torch.int32, device=queries.device)
    check(L.tt_bruteforce_search(index.data_ptr(), cand.data_ptr(), ldc, n, d, queries.data_ptr(), ldq, nq, k,
                                 index_offset, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _stream()))
    return out_s, out_i


def bruteforce_shard_chunk(n_queries: int, shard_sizes: Sequence[int], dim: int, k: int) -> int:
    """The query chunk every rank of a candidate-sharded search uses: the
    smallest of the shards' recommendations (tt_bruteforce_shard_chunk), so
    all ranks make the same number of all_reduce calls with the same lengths."""
    L = lib()
    return max(1, min(int(L.tt_bruteforce_shard_chunk(max(int(n_queries), 1), int(n), dim, k)) for n in shard_sizes))


def bruteforce_shard_search(index: torch.Tensor, cand: torch.Tensor, queries: torch.Tensor, k: int,
                            index_offset: int, reduce_max, chunk: Optional[int] = None
                            ) -> Tuple[torch.Tensor, torch.Tensor]:
    """This shard's part of a candidate-sharded exact top-k (tt.h
    tt_bruteforce_shard_*): per chunk of queries, the screen's lower bound on
    the shard's k-th score, `reduce_max(t)` (in place: the max over the shards,
    an all_reduce) as the floor, then the shard's exact top-k of the entries
    that can reach it, padded with (-inf, INT32_MAX).  `chunk` must be the
    same on every rank (bruteforce_shard_chunk over all shard sizes); the
    default, this shard's own recommendation, is only safe for one rank."""
    _req(index, "index", torch.uint8, 1)
    _req(cand, "cand", torch.float32, 2)
    _req(queries, "queries", torch.float32, 2)
    ldc, ldq = _row_major(cand, "cand"), _row_major(queries, "queries")
    n, d = cand.shape
    nq = queries.shape[0]
    if queries.shape[1] != d:
        raise ValueError("queries and candidates must share the embedding size")
    if k > n:
        raise ValueError(f"k={k} exceeds the shard's {n} candidates")
    L = lib()
    out_s = torch.empty(nq, k, dtype=torch.float32, device=queries.device)
    out_i = torch.empty(nq, k, dtype=torch.int32, device=queries.device)
    if nq == 0:
        return out_s, out_i
    chunk = int(chunk) if chunk else int(L.tt_bruteforce_shard_chunk(nq, n, d, k))
    if chunk < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    ws = Workspace.get(L.tt_bruteforce_shard_workspace_size(chunk, n, d, k), queries.device, "bruteforce_shard")
    kth = torch.empty(chunk, dtype=torch.float32, device=queries.device)
    for q0 in range(0, nq, chunk):
        m = min(chunk, nq - q0)
        qc = queries[q0:q0 + m]
        check(L.tt_bruteforce_shard_screen(index.data_ptr(), n, d, qc.data_ptr(), ldq, m, chunk, k, index_offset,
                                           kth.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        reduce_max(kth[:m])
        check(L.tt_bruteforce_shard_finalize(index.data_ptr(), cand.data_ptr(), ldc, n, d, qc.data_ptr(), ldq, m,
                                             chunk, k, index_offset, kth.data_ptr(), out_s[q0:q0 + m].data_ptr(),
                                             out_i[q0:q0 + m].data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return out_s, out_i


def topk_merge(scores: torch.Tensor, idx: torch.Tensor, k_out: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """scores/idx: [L, Q, k_in] sorted per list -> global [Q, k_out]."""
    _req(scores, "scores", torch.float32, 3)
    _req(idx, "idx", torch.int32, 3)
    if not (scores.is_contiguous() and idx.is_contiguous()) or scores.shape != idx.shape:
        raise ValueError("scores/idx must be contiguous and of equal shape")
    Ln, Q, k_in = scores.shape
    out_s = torch.empty(Q, k_out, dtype=torch.float32, device=scores.device)
    out_i = torch.empty(Q, k_out, dtype=torch.int32, device=scores.device)
    check(lib().tt_topk_merge(scores.data_ptr(), idx.data_ptr(), Ln, Q, k_in, k_out, out_s.data_ptr(),
                              out_i.data_ptr(), _stream()))
    return out_s, out_i


def topk_exclude(scores: torch.Tensor, idx: torch.Tensor, excl_off: torch.Tensor, excl_idx: torch.Tensor,
                 k_out: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Sorted lists scores/idx [Q, k_in] without each query's excluded
    candidates, compacted to k_out (tt_topk_exclude): query q's exclusions
    are excl_idx[excl_off[q]:excl_off[q+1]] (excl_off int64 [Q+1], device,
    non-decreasing, every offset within excl_idx — not checked here, that
    would synchronise; excl_idx int32, any order).  Returns (scores [Q, k_out],
    idx [Q, k_out], n_kept [Q] int32); rows with fewer than k_out entries left
    are padded with (-inf, INT32_MAX)."""
    _req(scores, "scores", torch.float32, 2)
    _req(idx, "idx", torch.int32, 2)
    _req(excl_off, "excl_off", torch.int64, 1)
    _req(excl_idx, "excl_idx", torch.int32, 1)
    if not (scores.is_contiguous() and idx.is_contiguous()) or scores.shape != idx.shape:
        raise ValueError("scores/idx must be contiguous and of equal shape")
    Q, k_in = scores.shape
    if excl_off.numel() != Q + 1 or not (excl_off.is_contiguous() and excl_idx.is_contiguous()):
        raise ValueError(f"excl_off must be a contiguous [{Q + 1}] int64 tensor and excl_idx contiguous")
    for t, name in ((idx, "idx"), (excl_off, "excl_off"), (excl_idx, "excl_idx")):
        if t.device != scores.device:
            raise ValueError(f"{name} must live on the scores' device {scores.device} (got {t.device})")
    k_out = int(k_out)
    if not 1 <= k_out <= k_in:
        raise ValueError(f"need 1 <= k_out <= k_in = {k_in}, got k_out={k_out}")
    out_s = torch.empty(Q, k_out, dtype=torch.float32, device=scores.device)
    out_i = torch.empty(Q, k_out, dtype=torch.int32, device=scores.device)
    kept = torch.empty(Q, dtype=torch.int32, device=scores.device)
    check(lib().tt_topk_exclude(scores.data_ptr(), idx.data_ptr(), Q, k_in, k_out, excl_off.data_ptr(),
                                excl_idx.data_ptr() if excl_idx.numel() else None, out_s.data_ptr(),
                                out_i.data_ptr(), kept.data_ptr(), _stream()))
    return out_s, out_i, kept


def recall_hits(true_ids: torch.Tensor, cand_ids: torch.Tensor, ks: Sequence[int], hits: torch.Tensor) -> None:
    """hits [len(ks)] int64 += #{b: true_ids[b] in cand_ids[b,:k]} (every match counts)."""
    _req(true_ids, "true_ids", torch.int32, 1)
    _req(cand_ids, "cand_ids", torch.int32, 2)
    _req(hits, "hits", torch.int64, 1)
    B, K = cand_ids.shape
    if true_ids.numel() != B or not cand_ids.is_contiguous() or not true_ids.is_contiguous():
        raise ValueError("true_ids [B] and cand_ids [B,K] must be contiguous")
    ks_arr = (ctypes.c_int32 * len(ks))(*[int(k) for k in ks])
    check(lib().tt_recall_hits(true_ids.data_ptr(), cand_ids.data_ptr(), B, K, ks_arr, len(ks), hits.data_ptr(),
                               _stream()))


_RANK_TABLES: Dict[Tuple[int, int], Tuple[torch.Tensor, torch.Tensor]] = {}


def rank_discount_tables(k_list: int) -> Tuple["np.ndarray", "np.ndarray"]:
    """Host fp32 tables of tt_rank_metrics: disc[i] = float32(1 / log2(i + 2))
    (computed in float64, rounded once) for i < k_list, and idcg[n] = the
    sequential fp32 sum of disc[:n] (idcg[0] = 0), n <= k_list."""
    import numpy as np

    disc = (1.0 / np.log2(np.arange(k_list, dtype=np.float64) + 2.0)).astype(np.float32)
    idcg = np.zeros(k_list + 1, np.float32)
    np.cumsum(disc, dtype=np.float32, out=idcg[1:])  # cumsum is sequential: one fp32 add per element
    return disc, idcg


def _rank_tables(device: torch.device, k_list: int) -> Tuple[torch.Tensor, torch.Tensor]:
    key = (device.index if device.index is not None else torch.cuda.current_device(), k_list)
    if key not in _RANK_TABLES:
        disc, idcg = rank_discount_tables(k_list)
        _RANK_TABLES[key] = (torch.as_tensor(disc, device=device), torch.as_tensor(idcg, device=device))
    return _RANK_TABLES[key]


def rank_metrics(cand: torch.Tensor, truth: torch.Tensor, ks: Sequence[int],
                 acc: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Set-valued ranking metrics (tt_rank_metrics) of ranked lists cand
    [Q, k_list] int32 against truth [Q, T] (or [Q]: T = 1) int32; values < 0
    or == INT32_MAX are padding on either side.  Rows may be strided (unit
    column stride).  Returns (vals [Q, len(ks), 4] fp32 = recall, ap, ndcg, rr
    at each k; hits [Q, len(ks)] int32; m [Q] int32 = distinct valid truth
    ids).  acc = (acc_f64 [len(ks), 4] float64, acc_i64 [len(ks), 2] int64,
    n_valid [1] int64) is added to: the sums of the four values, of hits and
    of the queries with a hit, and the number of queries with m > 0 (queries
    with m = 0 are in no sum)."""
    _req(cand, "cand", torch.int32, 2)
    if isinstance(truth, torch.Tensor) and truth.dim() == 1:
        truth = truth.unsqueeze(1)
    _req(truth, "truth", torch.int32, 2)
    if truth.device != cand.device:
        raise ValueError(f"truth must live on cand's device {cand.device} (got {truth.device})")
    Q, k_list = cand.shape
    T = truth.shape[1]
    if truth.shape[0] != Q:
        raise ValueError(f"truth has {truth.shape[0]} rows, cand {Q}")
    if not 1 <= k_list <= 4096 or not 1 <= T <= 1024:
        raise ValueError(f"need 1 <= k_list <= 4096 and 1 <= T <= 1024, got k_list={k_list}, T={T}")
    ks = [int(k) for k in ks]
    if not 1 <= len(ks) <= 16 or any(not 1 <= k <= k_list for k in ks):
        raise ValueError(f"need 1 to 16 values of k, each in [1, {k_list}], got {ks}")
    ld_cand, ld_truth = _row_major(cand, "cand"), _row_major(truth, "truth")
    nk = len(ks)
    ptrs = [None, None, None]
    if acc is not None:
        acc_f64, acc_i64, n_valid = acc
        _req(acc_f64, "acc_f64", torch.float64)
        _req(acc_i64, "acc_i64", torch.int64)
        _req(n_valid, "n_valid", torch.int64)
        for t, name, n in ((acc_f64, "acc_f64", 4 * nk), (acc_i64, "acc_i64", 2 * nk), (n_valid, "n_valid", 1)):
            if t.numel() != n or not t.is_contiguous() or t.device != cand.device:
                raise ValueError(f"{name} must be contiguous with {n} elements on {cand.device}")
        ptrs = [acc_f64.data_ptr(), acc_i64.data_ptr(), n_valid.data_ptr()]
    disc, idcg = _rank_tables(cand.device, k_list)
    vals = torch.empty(Q, nk, 4, dtype=torch.float32, device=cand.device)
    hits = torch.empty(Q, nk, dtype=torch.int32, device=cand.device)
    m = torch.empty(Q, dtype=torch.int32, device=cand.device)
    ks_arr = (ctypes.c_int32 * nk)(*ks)
    check(lib().tt_rank_metrics(cand.data_ptr(), ld_cand, k_list, truth.data_ptr(), ld_truth, T, Q, ks_arr, nk,
                                disc.data_ptr(), idcg.data_ptr(), vals.data_ptr(), hits.data_ptr(), m.data_ptr(),
                                ptrs[0], ptrs[1], ptrs[2], _stream()))
    return vals, hits, m


def batch_take(src: torch.Tensor, perm: torch.Tensor, cursor: torch.Tensor, out: torch.Tensor,
               advance: bool = True, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[c, b] = src[c, perm[cursor + b]] for the 32-bit word columns of an
    HBM-resident dataset (tt_batch_take); cursor (device int64 [1]) advances by
    the batch when `advance`.  Graph-capturable: nothing is read on the host."""
    _req(src, "src", torch.int32, 2)
    _req(perm, "perm", torch.int64, 1)
    _req(cursor, "cursor", torch.int64, 1)
    _req(out, "out", torch.int32, 2)
    if src.shape[0] != out.shape[0]:
        raise ValueError(f"src has {src.shape[0]} columns, out {out.shape[0]}")
    if perm.numel() != src.shape[1]:
        raise ValueError(f"perm has {perm.numel()} entries for {src.shape[1]} rows")
    if status is not None:
        _req(status, "status", torch.int32, 1)
    check(lib().tt_batch_take(src.data_ptr(), _row_major(src, "src"), src.shape[0], perm.data_ptr(), src.shape[1],
                              cursor.data_ptr(), out.shape[1], int(bool(advance)), out.data_ptr(),
                              _row_major(out, "out"), status.data_ptr() if status is not None else None,
                              _stream()))
    return out


def mixed_candidates(batch_cols: Sequence[torch.Tensor], cat: torch.Tensor, m: int, seed: int, step: torch.Tensor,
                     out: torch.Tensor, status: Optional[torch.Tensor] = None, n_cat: Optional[int] = None
                     ) -> torch.Tensor:
    """Mixed negative sampling, the candidate side of one step
    (tt_mixed_candidates): out[f, :B] = batch_cols[f], out[f, B + j] =
    cat[f, s_j] with the m rows s_j drawn uniformly from the catalogue's
    n_cat rows (default: all of cat's) by Philox4x32-10 at (seed, *step).
    batch_cols: one contiguous [B] column of 32-bit words (int32 / float32)
    per catalogue column; cat, out: int32 [F, N] / [F, >= B + m]; step: device
    int64 [1], left at step + 1.  Graph-capturable: nothing is read on the
    host, and every replay draws fresh rows."""
    _req(cat, "cat", torch.int32, 2)
    _req(out, "out", torch.int32, 2)
    _req(step, "step", torch.int64, 1)
    F = cat.shape[0]
    if len(batch_cols) != F or out.shape[0] != F:
        raise ValueError(f"the catalogue has {F} columns, the batch {len(batch_cols)}, out {out.shape[0]}")
    B = batch_cols[0].numel()
    for i, t in enumerate(batch_cols):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.float32):
            raise TypeError(f"batch column {i} must be an int32 or float32 tensor")
        if t.dim() != 1 or t.numel() != B or not t.is_contiguous() or t.device != cat.device:
            raise ValueError(f"batch column {i} must be a contiguous [{B}] tensor on {cat.device}")
    m = int(m)
    if m < 1:
        raise ValueError(f"m={m} must be >= 1")
    if out.shape[1] < B + m:
        raise ValueError(f"out has {out.shape[1]} slots for {B} + {m}")
    if status is not None:
        _req(status, "status", torch.int32, 1)
    ptrs = (ctypes.c_void_p * F)(*[t.data_ptr() for t in batch_cols])
    check(lib().tt_mixed_candidates(ptrs, cat.data_ptr(), _row_major(cat, "cat"), F, B, m,
                                    cat.shape[1] if n_cat is None else int(n_cat), int(seed) & (2 ** 64 - 1),
                                    step.data_ptr(), out.data_ptr(), _row_major(out, "out"),
                                    status.data_ptr() if status is not None else None, _stream()))
    return out


def mlp_pack(w: torch.Tensor, trans: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 hi/lo MFMA-fragment image of B = w ([K, N]) or B = w^T (trans:
    w is [N, K]) for mlp_rows (tt_mlp_pack)."""
    _req(w, "w", torch.float32, 2)
    K, N = (w.shape[1], w.shape[0]) if trans else (w.shape[0], w.shape[1])
    nbytes = lib().tt_mlp_pack_bytes(K, N)
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    if out.numel() < nbytes:
        raise ValueError(f"image buffer of {out.numel()} B < {nbytes} B")
    check(lib().tt_mlp_pack(w.data_ptr(), _row_major(w, "w"), K, N, int(bool(trans)), out.data_ptr(), out.numel(),
                            _stream()))
    out.mlp_kn = (K, N)
    return out


def score_matrix(q: torch.Tensor, c: torch.Tensor, chunk: int = 256) -> torch.Tensor:
    """S = q . c^T [Q, N] fp32 (TwoTowerModel.call, two_tower_model.py:92)
    on libtt's bf16x3 row GEMM: c in column chunks of `chunk` candidates, each
    packed as the B image of one tt_mlp_rows call writing its columns of S."""
    _req(q, "q", torch.float32, 2)
    _req(c, "c", torch.float32, 2)
    Q, E = q.shape
    N = c.shape[0]
    if c.shape[1] != E:
        raise ValueError(f"q {tuple(q.shape)} and c {tuple(c.shape)} must share the embedding size")
    n4 = (N + 3) // 4 * 4
    out = torch.empty(Q, max(n4, 4), dtype=torch.float32, device=q.device)
    if Q == 0 or N == 0:
        return out[:, :N]
    e4 = (E + 3) // 4 * 4
    a = q.contiguous()
    if e4 != E:  # 16-B rows for the kernel's vector loads
        a = torch.zeros(Q, e4, dtype=torch.float32, device=q.device)
        a[:, :E] = q
    cc = c.contiguous()
    for j0 in range(0, N, chunk):
        j1 = min(N, j0 + chunk)
        img = mlp_pack(cc[j0:j1], trans=True)
        mlp_rows(a, img, E, j1 - j0, out[:, j0:j1])
    return out[:, :N]


def matmul_rows(a: torch.Tensor, b: torch.Tensor, chunk: int = 256) -> torch.Tensor:
    """a [M, K] . b [K, N] fp32 on libtt's bf16x3 row GEMM (tt_mlp_rows) for
    any K and N: b in (K-chunk x N-chunk) blocks of <= `chunk`, each packed as
    one B image; the K-chunk partials of an output block are added in chunk
    order (deterministic).  The backward GEMMs of ScoreMatrix."""
    _req(a, "a", torch.float32, 2)
    _req(b, "b", torch.float32, 2)
    M, K = a.shape
    if b.shape[0] != K:
        raise ValueError(f"a {tuple(a.shape)} and b {tuple(b.shape)} do not chain")
    N = b.shape[1]
    out = torch.zeros(M, max((N + 3) // 4 * 4, 4), dtype=torch.float32, device=a.device)
    if M == 0 or N == 0 or K == 0:
        return out[:, :N]
    k4 = (K + 3) // 4 * 4
    aa = a.contiguous()
    if k4 != K:  # 16-B rows (and 16-B aligned column chunks) for the kernel's vector loads
        aa = torch.zeros(M, k4, dtype=torch.float32, device=a.device)
        aa[:, :K] = a
    bb = b.contiguous()
    part = torch.empty(M, min(chunk, (N + 3) // 4 * 4), dtype=torch.float32, device=a.device)
    for n0 in range(0, N, chunk):
        n1 = min(N, n0 + chunk)
        for k0 in range(0, K, chunk):
            k1 = min(K, k0 + chunk)
            img = mlp_pack(bb[k0:k1, n0:n1].contiguous())
            mlp_rows(aa[:, k0:], img, k1 - k0, n1 - n0, part)
            out[:, n0:n1] += part[:, :n1 - n0]
    return out[:, :N]


class ScoreMatrix(torch.autograd.Function):
    """S = q . c^T with its gradients, every product on libtt (score_matrix
    forward; dq = G . c and dc = G^T . q by matmul_rows): the differentiable
    form of TwoTowerModel.call (two_tower_model.py:92, tf.matmul)."""

    @staticmethod
    def forward(ctx, q, c):
        ctx.save_for_backward(q, c)
        return score_matrix(q.detach(), c.detach())

    @staticmethod
    def backward(ctx, g):
        q, c = ctx.saved_tensors
        g = g.contiguous()
        dq = matmul_rows(g, c.detach()) if ctx.needs_input_grad[0] else None
        dc = matmul_rows(g.t().contiguous(), q.detach()) if ctx.needs_input_grad[1] else None
        return dq, dc


def _pack_job_array(jobs: Sequence[Tuple[torch.Tensor, bool, torch.Tensor]]):
    arr = (_native.MlpPackJob * len(jobs))()
    for i, (w, trans, img) in enumerate(jobs):
        _req(w, "w", torch.float32, 2)
        K, N = (w.shape[1], w.shape[0]) if trans else (w.shape[0], w.shape[1])
        arr[i].w, arr[i].ldw, arr[i].K, arr[i].N = w.data_ptr(), _row_major(w, "w"), K, N
        arr[i].trans, arr[i].img, arr[i].img_bytes = int(bool(trans)), img.data_ptr(), img.numel()
    return arr


def mlp_pack_many(jobs: Sequence[Tuple[torch.Tensor, bool, torch.Tensor]]) -> None:
    """Several mlp_pack images in one launch: jobs of (w, trans, image buffer)."""
    check(lib().tt_mlp_pack_many(_pack_job_array(jobs), len(jobs), _stream()))


def _check_rows(a, k, n, out, amask, cmask, bias) -> int:
    """mlp_rows' operand checks; returns M."""
    _req(a, "a", torch.float32, 2)
    _req(out, "out", torch.float32, 2)
    M = a.shape[0]
    if a.shape[1] < k or out.shape[0] != M or out.shape[1] < n:
        raise ValueError(f"mlp_rows: a {tuple(a.shape)}, out {tuple(out.shape)}, k={k}, n={n}")
    for t, nm in ((amask, "amask"), (cmask, "cmask")):
        if t is not None:
            _req(t, nm, torch.float32, 2)
            if t.shape[0] != M:
                raise ValueError(f"{nm} has {t.shape[0]} rows, expected {M}")
    if amask is not None and amask.shape[1] < k:
        raise ValueError("amask narrower than k")
    if cmask is not None and cmask.shape[1] < n:
        raise ValueError("cmask narrower than n")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() < n or not bias.is_contiguous()):
        raise ValueError("bias must be a contiguous fp32 vector of >= n entries")
    return M


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def mlp_rows(a: torch.Tensor, img: torch.Tensor, k: int, n: int, out: torch.Tensor, *,
             amask: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
             bias: Optional[torch.Tensor] = None, relu: bool = False,
             cmask: Optional[torch.Tensor] = None, colsum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M, n] = epi(maskA(a[:, :k]) . B) with B packed by mlp_pack (tt_mlp_rows);
    colsum (a contiguous [n] tensor): also the column sums of out.  n <= 4096
    (over 384 the one launch covers column groups, same arithmetic)."""
    M = _check_rows(a, k, n, out, amask, cmask, bias)
    ws = None
    if colsum is not None:
        if colsum.dtype != torch.float32 or colsum.numel() != n or not colsum.is_contiguous():
            raise ValueError("colsum must be a contiguous fp32 [n] tensor")
        ws = Workspace.get(lib().tt_mlp_rows_workspace_size(M, n), a.device, "mlp_colsum")
    check(lib().tt_mlp_rows(a.data_ptr(), _row_major(a, "a"), _ptr(amask),
                            _row_major(amask, "amask") if amask is not None else 0,
                            _ptr(scale), M, k, img.data_ptr(), n, _ptr(bias), int(bool(relu)), _ptr(cmask),
                            _row_major(cmask, "cmask") if cmask is not None else 0, out.data_ptr(),
                            _row_major(out, "out"), _ptr(colsum), _ptr(ws), ws.numel() if ws is not None else 0,
                            _stream()))
    return out


def mlp_rows_pair(problems: Sequence[dict]) -> None:
    """Two independent mlp_rows problems (the two towers' layers) in ONE
    launch (tt_mlp_rows_pair); each problem is a dict of mlp_rows' arguments
    a, img, k, n, out and optionally amask, scale, bias, relu, cmask (no
    colsum).  Results equal two mlp_rows calls bit for bit."""
    if len(problems) != 2:
        raise ValueError("mlp_rows_pair takes exactly 2 problems")
    arr = (_native.MlpRowsProblem * 2)()
    for i, p in enumerate(problems):
        _fill_rows_problem(arr[i], p)
    check(lib().tt_mlp_rows_pair(arr, _stream()))


def _fill_rows_problem(q, p: dict) -> None:
    """A tt_mlp_rows_problem from a dict of mlp_rows' arguments (no colsum)."""
    a, img, k, n, out = p["a"], p["img"], p["k"], p["n"], p["out"]
    amask, cmask, bias = p.get("amask"), p.get("cmask"), p.get("bias")
    M = _check_rows(a, k, n, out, amask, cmask, bias)
    q.A, q.lda, q.amask = a.data_ptr(), _row_major(a, "a"), _ptr(amask)
    q.ldam = _row_major(amask, "amask") if amask is not None else 0
    q.scale, q.M, q.K, q.img, q.N = _ptr(p.get("scale")), M, k, img.data_ptr(), n
    q.bias, q.relu, q.cmask = _ptr(bias), int(bool(p.get("relu", False))), _ptr(cmask)
    q.ldcm = _row_major(cmask, "cmask") if cmask is not None else 0
    q.C, q.ldc = out.data_ptr(), _row_major(out, "out")


def _check_wgrad(a, g, dwb, gmask) -> Tuple[int, int, int]:
    _req(a, "a", torch.float32, 2)
    _req(g, "g", torch.float32, 2)
    _req(dwb, "dwb", torch.float32, 2)
    M, Ka = a.shape
    N = g.shape[1]
    if g.shape[0] != M or tuple(dwb.shape) != (Ka + 1, N) or not dwb.is_contiguous():
        raise ValueError(f"mlp_wgrad: a {tuple(a.shape)}, g {tuple(g.shape)}, dwb {tuple(dwb.shape)}")
    if gmask is not None:
        _req(gmask, "gmask", torch.float32, 2)
        if tuple(gmask.shape) != (M, N):
            raise ValueError("gmask must match g")
    return M, Ka, N


def mlp_wgrad(a: torch.Tensor, g: torch.Tensor, dwb: torch.Tensor, *, gmask: Optional[torch.Tensor] = None,
              scale: Optional[torch.Tensor] = None, adagrad: Optional[tuple] = None) -> torch.Tensor:
    """dwb [Ka + 1, N] = [a | 1]^T . Gm (weight gradient rows then the bias
    gradient row), Gm = g or (gmask > 0) ? g * scale : 0 (tt_mlp_wgrad).
    adagrad = (param, accum, lr, eps): also the layer's Adagrad step on
    param / accum (contiguous, dwb's shape) from the summed gradient
    (tt_mlp_wgrad_adagrad: dense_adagrad's arithmetic inside the sum launch)."""
    M, Ka, N = _check_wgrad(a, g, dwb, gmask)
    ws = Workspace.get(lib().tt_mlp_wgrad_workspace_size(M, Ka, N), a.device, "mlp_wgrad")
    args = (a.data_ptr(), _row_major(a, "a"), g.data_ptr(), _row_major(g, "g"), _ptr(gmask),
            _row_major(gmask, "gmask") if gmask is not None else 0, _ptr(scale), M, Ka, N, dwb.data_ptr())
    if adagrad is not None:
        check(lib().tt_mlp_wgrad_adagrad(*args, *_adagrad_args(adagrad, dwb), ws.data_ptr(), ws.numel(), _stream()))
        return dwb
    check(lib().tt_mlp_wgrad(*args, ws.data_ptr(), ws.numel(), _stream()))
    return dwb


def _adagrad_args(adagrad, dwb: torch.Tensor):
    param, accum, lr, eps = adagrad
    for t, n in ((param, "param"), (accum, "accum")):
        _req(t, n, torch.float32)
        if t.numel() != dwb.numel() or not t.is_contiguous():
            raise ValueError(f"{n} must be contiguous with dwb's {dwb.numel()} elements")
    return param.data_ptr(), accum.data_ptr(), float(lr), float(eps)


def mlp_wgrad_job(a: torch.Tensor, g: torch.Tensor, dwb: torch.Tensor, *, gmask: Optional[torch.Tensor] = None,
                  scale: Optional[torch.Tensor] = None, adagrad: Optional[tuple] = None,
                  tag: str = "mlp_wgrad_job"):
    """mlp_wgrad's problem (and optional Adagrad step) as a tt_mlp_wgrad_job
    for mlp_backward_layer / mlp_wgrad_finish; its split partials live in
    the workspace `tag` (consecutive layers of one chain need different
    tags: a job's partials are summed by the NEXT launch)."""
    M, Ka, N = _check_wgrad(a, g, dwb, gmask)
    ws = Workspace.get(lib().tt_mlp_wgrad_workspace_size(M, Ka, N), a.device, tag)
    j = _native.MlpWgradJob()
    q = j.p
    q.A, q.lda, q.G, q.ldg = a.data_ptr(), _row_major(a, "a"), g.data_ptr(), _row_major(g, "g")
    q.gmask, q.ldgm = _ptr(gmask), _row_major(gmask, "gmask") if gmask is not None else 0
    q.scale, q.M, q.Ka, q.N, q.dwb = _ptr(scale), M, Ka, N, dwb.data_ptr()
    j.parts, j.parts_bytes = ws.data_ptr(), ws.numel()
    if adagrad is not None:
        j.param, j.accum, j.lr, j.eps = _adagrad_args(adagrad, dwb)
    return j


def mlp_backward_layer(job, rows: Optional[dict] = None, prev=None) -> Optional[torch.Tensor]:
    """One Dense layer's backward in ONE launch (tt_mlp_backward_layer): the
    weight-gradient partials of `job`, the input-gradient GEMM `rows` (a dict
    of mlp_rows' arguments, no colsum, n <= 384; None: none) and the partial
    sums (+ Adagrad) of the previous layer's job `prev`.  Returns rows["out"]."""
    r = None
    if rows is not None:
        r = _native.MlpRowsProblem()
        _fill_rows_problem(r, rows)
    check(lib().tt_mlp_backward_layer(ctypes.byref(job), ctypes.byref(r) if r is not None else None,
                                      ctypes.byref(prev) if prev is not None else None, _stream()))
    return rows["out"] if rows is not None else None


def mlp_wgrad_finish(job) -> None:
    """The partial sums (+ Adagrad) of the last job of a backward chain."""
    check(lib().tt_mlp_wgrad_finish(ctypes.byref(job), _stream()))


def mlp_wgrad_pair(problems: Sequence[dict]) -> None:
    """Two mlp_wgrad problems (dicts of a, g, dwb and optionally gmask,
    scale) in one launch plus one partial-sum launch (tt_mlp_wgrad_pair)."""
    if len(problems) != 2:
        raise ValueError("mlp_wgrad_pair takes exactly 2 problems")
    arr = (_native.MlpWgradProblem * 2)()
    for i, p in enumerate(problems):
        a, g, dwb, gmask = p["a"], p["g"], p["dwb"], p.get("gmask")
        M, Ka, N = _check_wgrad(a, g, dwb, gmask)
        q = arr[i]
        q.A, q.lda, q.G, q.ldg = a.data_ptr(), _row_major(a, "a"), g.data_ptr(), _row_major(g, "g")
        q.gmask, q.ldgm = _ptr(gmask), _row_major(gmask, "gmask") if gmask is not None else 0
        q.scale, q.M, q.Ka, q.N, q.dwb = _ptr(p.get("scale")), M, Ka, N, dwb.data_ptr()
    ws = Workspace.get(lib().tt_mlp_wgrad_pair_workspace_size(arr), problems[0]["a"].device, "mlp_wgrad")
    check(lib().tt_mlp_wgrad_pair(arr, ws.data_ptr(), ws.numel(), _stream()))


# --------------------------------------------------------------------------
# Cosine scoring: row L2 normalisation and its gradient
# --------------------------------------------------------------------------
def _norm_operand(t: torch.Tensor, name: str, rows: int, dim: int, like: torch.Tensor) -> int:
    """A [rows, dim] fp32 operand on like's device; returns its leading dimension."""
    _req(t, name, torch.float32, 2)
    if tuple(t.shape) != (rows, dim):
        raise ValueError(f"{name} must be [{rows}, {dim}], got {tuple(t.shape)}")
    if t.device != like.device:
        raise ValueError(f"{name} must live on {like.device} (got {t.device})")
    return _norm_ld(t, name)


def _norm_ld(t: torch.Tensor, name: str) -> int:
    """_row_major, refusing rows that overlap (a row stride below the width)."""
    ld = _row_major(t, name)
    if t.shape[0] > 1 and t.stride(0) < t.shape[1]:
        raise ValueError(f"{name}: row stride {t.stride(0)} below its width {t.shape[1]}")
    return ld


def _norm_inv(t: torch.Tensor, name: str, rows: int, like: torch.Tensor) -> None:
    _req(t, name, torch.float32, 1)
    if t.numel() != rows or not t.is_contiguous() or t.device != like.device:
        raise ValueError(f"{name} must be a contiguous [{rows}] float32 tensor on {like.device}")


def _norm_dim(x: torch.Tensor, name: str) -> Tuple[int, int]:
    _req(x, name, torch.float32, 2)
    rows, dim = x.shape
    if not 1 <= dim <= 4096:
        raise ValueError(f"{name}: dim={dim} outside 1..4096 (tt_l2norm_rows)")
    return rows, dim


def l2norm_rows(jobs: Sequence[tuple]) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """Row L2 normalisation of 1 or 2 operands in ONE launch (tt_l2norm_rows).
    Each job is (x, scale) or (x, scale, y, inv): x [rows, dim] fp32 with unit
    column stride (any row stride >= dim), y like x and inv [rows] contiguous
    (allocated when omitted or None).  y_i = x_i * scale / ||x_i||, inv_i =
    1 / ||x_i||; a zero row gives y_i = 0, inv_i = 0.  Returns [(y, inv)] per
    job.  A two-job call equals two one-job calls bit for bit."""
    if not 1 <= len(jobs) <= 2:
        raise ValueError("l2norm_rows takes 1 or 2 jobs")
    arr = (_native.L2NormJob * len(jobs))()
    out = []
    for i, job in enumerate(jobs):
        x, scale, y, inv = (tuple(job) + (None, None))[:4]
        rows, dim = _norm_dim(x, f"x[{i}]")
        ldx = _norm_ld(x, f"x[{i}]")
        if y is None:
            y = torch.empty(rows, dim, dtype=torch.float32, device=x.device)
        if inv is None:
            inv = torch.empty(rows, dtype=torch.float32, device=x.device)
        ldy = _norm_operand(y, f"y[{i}]", rows, dim, x)
        _norm_inv(inv, f"inv[{i}]", rows, x)
        q = arr[i]
        q.x, q.ldx, q.y, q.ldy, q.inv = x.data_ptr(), ldx, y.data_ptr(), ldy, inv.data_ptr()
        q.rows, q.dim, q.scale = rows, dim, float(scale)
        out.append((y, inv))
    check(lib().tt_l2norm_rows(arr, len(jobs), _stream()))
    return out


def l2norm_rows_grad(jobs: Sequence[tuple]) -> List[torch.Tensor]:
    """Gradient of l2norm_rows for 1 or 2 operands in ONE launch
    (tt_l2norm_rows_grad).  Each job is (x, inv, dy, scale) or (x, inv, dy,
    scale, dx): x the forward's input, inv its reciprocal norms, dy [rows,
    dim] the gradient with respect to y; dx may be dy itself (in place) and is
    allocated when omitted or None.  dx_i = scale inv_i (dy_i - u_i (u_i .
    dy_i)) with u_i = x_i inv_i; zero rows get dx_i = 0.  Returns [dx] per job."""
    if not 1 <= len(jobs) <= 2:
        raise ValueError("l2norm_rows_grad takes 1 or 2 jobs")
    arr = (_native.L2NormGradJob * len(jobs))()
    out = []
    for i, job in enumerate(jobs):
        x, inv, dy, scale, dx = (tuple(job) + (None,))[:5]
        rows, dim = _norm_dim(x, f"x[{i}]")
        ldx = _norm_ld(x, f"x[{i}]")
        _norm_inv(inv, f"inv[{i}]", rows, x)
        lddy = _norm_operand(dy, f"dy[{i}]", rows, dim, x)
        if dx is None:
            dx = torch.empty(rows, dim, dtype=torch.float32, device=x.device)
        lddx = _norm_operand(dx, f"dx[{i}]", rows, dim, x)
        q = arr[i]
        q.x, q.ldx, q.inv, q.dy, q.lddy = x.data_ptr(), ldx, inv.data_ptr(), dy.data_ptr(), lddy
        q.dx, q.lddx, q.rows, q.dim, q.scale = dx.data_ptr(), lddx, rows, dim, float(scale)
        out.append(dx)
    check(lib().tt_l2norm_rows_grad(arr, len(jobs), _stream()))
    return out


# --------------------------------------------------------------------------
# Sequence features: pooled embedding bags and their gradient expansion
# --------------------------------------------------------------------------
def _bag_ids(ids: torch.Tensor, name: str, batch: int, like: torch.Tensor) -> Tuple[int, int, int]:
    """ids [batch, L] int32 with any (non-negative) strides -> (L, row stride, slot stride)."""
    _req(ids, name, torch.int32, 2)
    if ids.shape[0] != batch or ids.device != like.device:
        raise ValueError(f"{name} must be [{batch}, L] int32 on {like.device}, got {tuple(ids.shape)} on {ids.device}")
    if ids.stride(0) < 0 or ids.stride(1) < 0:
        raise ValueError(f"{name}: negative strides are not supported")
    return ids.shape[1], ids.stride(0), ids.stride(1)


def _bag_pooling(pooling: str) -> int:
    if pooling not in _native.BAG_POOLINGS:
        raise ValueError(f"pooling must be one of {sorted(_native.BAG_POOLINGS)}, got {pooling!r}")
    return _native.BAG_POOLINGS[pooling]


def _bag_scale(t: torch.Tensor, name: str, batch: int, like: torch.Tensor) -> None:
    _req(t, name, torch.float32, 1)
    if t.numel() != batch or not t.is_contiguous() or t.device != like.device:
        raise ValueError(f"{name} must be a contiguous [{batch}] float32 tensor on {like.device}")


def gather_bag(jobs: Sequence[tuple], batch: int) -> None:
    """Pooled embedding bags of 1..8 sequence features in ONE launch
    (tt_gather_bag).  Each job is (table [V, D], ids [batch, L] int32 with any
    strides, pooling "sum" | "mean" | "sqrtn", out [batch, >= col_offset + D]
    fp32 with unit column stride, col_offset, scale_out [batch]): columns
    [col_offset, col_offset + D) of out receive the pooled rows of the valid
    slots (0 <= id < V; -1 pads), scale_out the factor applied (0 for an empty
    bag).  The other columns of out are not touched."""
    if not 1 <= len(jobs) <= _native.MAX_BAG_JOBS:
        raise ValueError(f"gather_bag takes 1..{_native.MAX_BAG_JOBS} jobs")
    arr = (_native.BagJob * len(jobs))()
    for i, (table, ids, pooling, out, off, scale_out) in enumerate(jobs):
        _req(table, f"table[{i}]", torch.float32, 2)
        if not table.is_contiguous():
            raise ValueError(f"table[{i}] must be contiguous")
        L, rs, ps = _bag_ids(ids, f"ids[{i}]", batch, table)
        _req(out, f"out[{i}]", torch.float32, 2)
        if out.shape[0] != batch or out.device != table.device:
            raise ValueError(f"out[{i}] must have {batch} rows on {table.device}")
        ld = _norm_ld(out, f"out[{i}]")
        if off < 0 or off + table.shape[1] > max(out.shape[1], 1):
            raise ValueError(f"out[{i}]: columns [{off}, {off + table.shape[1]}) outside its {out.shape[1]} columns")
        _bag_scale(scale_out, f"scale_out[{i}]", batch, table)
        q = arr[i]
        q.table, q.num_rows, q.dim, q.L = table.data_ptr(), table.shape[0], table.shape[1], L
        q.ids, q.ids_row_stride, q.ids_pos_stride = ids.data_ptr(), rs, ps
        q.pooling, q.col_offset = _bag_pooling(pooling), off
        q.out, q.out_stride, q.scale_out = out.data_ptr(), ld, scale_out.data_ptr()
    check(lib().tt_gather_bag(arr, len(jobs), batch, _stream()))


def bag_grad_expand(jobs: Sequence[tuple], batch: int) -> None:
    """The flat sparse problem of 1..8 bag features in ONE launch
    (tt_bag_grad_expand).  Each job is (num_rows, ids [batch, L], pooling,
    dout [batch, *], col_offset, scale [batch] from gather_bag, ids_flat
    [batch * L] int32, grad [batch * L, D] fp32 contiguous): ids_flat[b * L +
    l] is the slot's id or -1, and the grad row of every valid slot is
    dout[b, col_offset : col_offset + D] * scale[b].  Rows of invalid slots
    are not written."""
    if not 1 <= len(jobs) <= _native.MAX_BAG_JOBS:
        raise ValueError(f"bag_grad_expand takes 1..{_native.MAX_BAG_JOBS} jobs")
    arr = (_native.BagGradJob * len(jobs))()
    for i, (num_rows, ids, pooling, dout, off, scale, ids_flat, grad) in enumerate(jobs):
        _req(dout, f"dout[{i}]", torch.float32, 2)
        L, rs, ps = _bag_ids(ids, f"ids[{i}]", batch, dout)
        _req(grad, f"grad[{i}]", torch.float32, 2)
        dim = grad.shape[1]
        if grad.shape[0] != batch * L or not grad.is_contiguous() or grad.device != dout.device:
            raise ValueError(f"grad[{i}] must be a contiguous [{batch * L}, D] float32 tensor on {dout.device}")
        _req(ids_flat, f"ids_flat[{i}]", torch.int32, 1)
        if ids_flat.numel() != batch * L or not ids_flat.is_contiguous() or ids_flat.device != dout.device:
            raise ValueError(f"ids_flat[{i}] must be a contiguous [{batch * L}] int32 tensor on {dout.device}")
        if dout.shape[0] != batch or off < 0 or off + dim > dout.shape[1]:
            raise ValueError(f"dout[{i}] must be [{batch}, >= {off + dim}], got {tuple(dout.shape)}")
        ld = _norm_ld(dout, f"dout[{i}]")
        _bag_scale(scale, f"scale[{i}]", batch, dout)
        q = arr[i]
        q.num_rows, q.dim, q.L = int(num_rows), dim, L
        q.ids, q.ids_row_stride, q.ids_pos_stride = ids.data_ptr(), rs, ps
        q.pooling, q.col_offset = _bag_pooling(pooling), off
        q.dout, q.dout_stride, q.scale = dout.data_ptr(), ld, scale.data_ptr()
        q.ids_flat, q.grad = ids_flat.data_ptr(), grad.data_ptr()
    check(lib().tt_bag_grad_expand(arr, len(jobs), batch, _stream()))


# --------------------------------------------------------------------------
# Gradient clipping: clipvalue / clipnorm / global_clipnorm in place
# --------------------------------------------------------------------------
class ClipRegions(tuple):
    """clip_regions' result: (tt_clip_region array, count, device)."""


def clip_regions(regions: Sequence[tuple], num_vars: int) -> ClipRegions:
    """The tt_clip_region array of `regions`, each (g, row_ids, var): g a 1-D
    fp32 tensor with unit stride (one row) or a 2-D view with unit column
    stride and any row stride >= its width (a column range of a wider
    matrix); row_ids None or a contiguous [rows] int32 tensor (rows with id <
    0 are skipped); var in [0, num_vars).  An empty g is a region without
    values."""
    arr = (_native.ClipRegion * max(len(regions), 1))()
    dev = None
    for i, (g, row_ids, var) in enumerate(regions):
        _req(g, f"g[{i}]", torch.float32)
        if dev is not None and g.device != dev:
            raise ValueError(f"g[{i}] must live on {dev} (got {g.device})")
        dev = g.device
        if g.dim() == 1:
            if g.numel() > 1 and g.stride(0) != 1:
                raise ValueError(f"g[{i}] must have unit stride")
            rows, cols, ld = 1, g.numel(), g.numel()
        elif g.dim() == 2:
            rows, cols = g.shape
            ld = _norm_ld(g, f"g[{i}]")
        else:
            raise ValueError(f"g[{i}] must be 1-D or 2-D, got shape {tuple(g.shape)}")
        if cols >= 1 << 31:
            raise ValueError(f"g[{i}]: {cols} columns do not fit an int32")
        if not 0 <= int(var) < num_vars:
            raise ValueError(f"region {i}: var={var} outside [0, {num_vars})")
        q = arr[i]
        q.g, q.rows, q.cols, q.ld, q.var = g.data_ptr(), rows, cols, ld, int(var)
        q.row_ids = None
        if row_ids is not None:
            _req(row_ids, f"row_ids[{i}]", torch.int32, 1)
            if row_ids.numel() != rows or not row_ids.is_contiguous() or row_ids.device != g.device:
                raise ValueError(f"row_ids[{i}] must be a contiguous [{rows}] int32 tensor on {g.device}")
            q.row_ids = row_ids.data_ptr()
    return ClipRegions((arr, len(regions), dev))


def _clip_out(t: torch.Tensor, name: str, dtype: torch.dtype, num_vars: int, dev) -> None:
    _req(t, name, dtype, 1)
    if t.numel() != num_vars or not t.is_contiguous() or (dev is not None and t.device != dev):
        raise ValueError(f"{name} must be a contiguous [{num_vars}] {dtype} tensor on the gradients' device")


def grad_sumsq(regions, num_vars: int, clipvalue: Optional[float], sumsq: torch.Tensor,
               ws_tag: str = "grad_clip") -> None:
    """sumsq[v] (fp64, [num_vars]) = the sum of squares of variable v's values
    after the clipvalue clamp (None: no clamp), tt_grad_sumsq: fp64 from exact
    products in a fixed order.  `regions`: clip_regions' input or its result."""
    arr, n, dev = regions if isinstance(regions, ClipRegions) else clip_regions(regions, num_vars)
    _clip_out(sumsq, "sumsq", torch.float64, num_vars, dev)
    need = lib().tt_grad_clip_workspace_size(arr, n)
    if need == 0:
        raise ValueError("grad_sumsq: a region is too large")
    ws = Workspace.get(need, sumsq.device, ws_tag)
    check(lib().tt_grad_sumsq(arr, n, num_vars, float(clipvalue or 0.0), sumsq.data_ptr(), ws.data_ptr(),
                              ws.numel(), _stream()))


def grad_clip_apply(regions, num_vars: int, clipvalue: Optional[float], clipnorm: Optional[float],
                    global_clipnorm: Optional[float], sumsq: Optional[torch.Tensor],
                    factor: Optional[torch.Tensor]) -> None:
    """g <- clamp(g, +-clipvalue) * f in place over every region
    (tt_grad_clip_apply), f = c / max(fp32(sqrt(ss)), c) from sumsq per
    variable (clipnorm) or over all variables (global_clipnorm), 1 with
    neither; factor[v] (fp32, [num_vars]) receives f when given."""
    arr, n, dev = regions if isinstance(regions, ClipRegions) else clip_regions(regions, num_vars)
    if sumsq is not None:
        _clip_out(sumsq, "sumsq", torch.float64, num_vars, dev)
    elif clipnorm or global_clipnorm:
        raise ValueError("grad_clip_apply: a norm needs sumsq")
    if factor is not None:
        _clip_out(factor, "factor", torch.float32, num_vars, dev)
    check(lib().tt_grad_clip_apply(arr, n, num_vars, float(clipvalue or 0.0), float(clipnorm or 0.0),
                                   float(global_clipnorm or 0.0), sumsq.data_ptr() if sumsq is not None else None,
                                   factor.data_ptr() if factor is not None else None, _stream()))
