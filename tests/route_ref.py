"""The request-routing contract of include/tt.h (tt_route_requests,
tt_route_requests_ordered, tt_route_pad, tt_route_owner, tt_route_fixed) as a
numpy checker, and the case list the host and GPU tests share.

The checker restates the header, not the kernels: every output is an integer
array with a complete specification, so each check_* function states the
conditions of the header and raises RouteMismatch at the first one an answer
breaks.  The request conditions (distinct (row, tag) pairs, strictly
increasing in (owner, tag, row), counts per owner, every lookup names its own
request, every request is named) admit exactly one answer; reference() builds
that answer with np.unique and passes it through check_requests before anyone
uses it, and the padded check states the slots against it.

The cases are data: name, world, num_tags, the lookups (table rows, tag), the
batch, how the ids are made and the path tt_route_fixed must take for them
(`fused`: one workgroup; `multi32` / `multi64`: key build + device sort +
heads + write (+ pad) with 32- or 64-bit keys), which route_path() recomputes
from plan_route's bit count.  The sizes around the fused limit are written in
terms of kRsMax, read from the kernel source.
"""
import functools
import os
import re
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

INT32_MAX = 2 ** 31 - 1
INT32_MIN = -2 ** 31

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hm-retrieval-two-tower_amd", "csrc",
                    "tt_route.hip")


def _constant(name: str) -> int:
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(_SRC).read()).group(1))


K_RS_MAX = _constant("kRsMax")                # lookups the one-workgroup route takes
K_MAX_WORLD = _constant("kMaxWorld")
K_MAX_LOOKUPS = _constant("kMaxRouteLookups")


class RouteMismatch(AssertionError):
    """An answer breaks a condition of the routing contract."""


def _fail(what: str, *args) -> None:
    raise RouteMismatch(what % args if args else what)


def _first(mask: np.ndarray) -> int:
    return int(np.flatnonzero(np.asarray(mask).reshape(-1))[0])


# --------------------------------------------------------------------------- plan_route's bit count
def bits_for(x: int) -> int:
    """Bits needed to represent the values 0..x."""
    b = 1
    while (1 << b) <= x:
        b += 1
    return b


def end_bit(world: int, num_tags: int, max_rows: int) -> int:
    """Width of the route's sort key (owner, tag, row + 1): row + 1 is at most
    max_rows, (owner, tag) at most world * num_tags - 1."""
    return bits_for(max_rows) + bits_for(world * num_tags - 1)


def route_path(total: int, world: int, num_tags: int, max_rows: int) -> str:
    e = end_bit(world, num_tags, max_rows)
    if total <= K_RS_MAX and e <= 32:
        return "fused"
    return "multi32" if e <= 32 else "multi64"


# --------------------------------------------------------------------------- the cases
class Case(NamedTuple):
    name: str
    world: int
    num_tags: int
    tables: Tuple[Tuple[int, int], ...]  # per lookup (table rows, tag); one row count per tag
    batch: int
    path: str                            # fused / multi32 / multi64: the path tt_route_fixed must take
    content: str = "mixed"               # how ids() fills the lookups
    seed: int = 0

    @property
    def total(self) -> int:
        return len(self.tables) * self.batch

    @property
    def max_rows(self) -> int:
        return max(r for r, _ in self.tables)

    @property
    def end_bit(self) -> int:
        return end_bit(self.world, self.num_tags, self.max_rows)

    def ids(self) -> List[np.ndarray]:
        """The lookups' ids ([batch] int32 each), built once per case; read-only."""
        return _case_ids(self)


def specials(rows: int) -> np.ndarray:
    s = [0, 1, rows - 2, rows - 1, rows, rows + 1, rows // 2, -1, -2, INT32_MAX, INT32_MIN]
    return np.clip(np.array(s, np.int64), INT32_MIN, INT32_MAX)


def mixed_ids(rng: np.random.Generator, n: int, rows: int) -> np.ndarray:
    """Half uniform in the table, half from the table's edges and outside it."""
    k = n // 2
    ids = np.concatenate([rng.integers(0, rows, n - k), rng.choice(specials(rows), k)])
    rng.shuffle(ids)
    return ids.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case_ids(case: Case) -> List[np.ndarray]:
    rng = np.random.default_rng(case.seed)
    B = case.batch
    if case.content == "mixed":
        ids = [mixed_ids(rng, B, rows) for rows, _ in case.tables]
        if B >= 3:  # a duplicate of a valid id and an id just past the table, whatever the draw gave
            p = rng.choice(B, 3, replace=False)
            rows = case.tables[0][0]
            ids[0][p[0]] = ids[0][p[1]] = rng.integers(0, rows)
            ids[0][p[2]] = rows
    elif case.content == "all_invalid":
        ids = [np.where(np.arange(B) % 2 == 0, rows, -1).astype(np.int32) for rows, _ in case.tables]
    elif case.content == "all_equal":
        ids = [np.full(B, rows - 1, np.int32) for rows, _ in case.tables]
    elif case.content == "all_distinct":
        ids = [rng.permutation(rows)[:B].astype(np.int32) for rows, _ in case.tables]
    else:
        raise ValueError(case.content)
    for x in ids:
        x.setflags(write=False)
    return ids


SIZE_ROWS = (5000, 700, 1371980)  # tags cycle over these tables
SIZE_WORLDS = (1, 3, 8)
C5_ROWS = 100_000_000


def _size_case(L: int, B: int, world: int, path: str) -> Case:
    tables = tuple((SIZE_ROWS[l % 3], l % 3) for l in range(L))
    return Case(f"{L}x{B}-w{world}", world, 3, tables, B, path, seed=1000 * L + B + world)


def _cases() -> List[Case]:
    K = K_RS_MAX
    fused = [(1, 1), (1, 2), (1, 63), (1, 64), (1, 65), (1, 1023), (1, 1024), (1, 1025), (3, K // 3), (1, K - 1),
             (1, K), (2, K // 2), (32, K // 32)]
    multi = [(1, K + 1), (3, K // 3 + 1), (32, K // 32 + 1)]
    out = [_size_case(L, B, w, "fused") for L, B in fused for w in SIZE_WORLDS]
    out += [_size_case(L, B, w, "multi32") for L, B in multi for w in SIZE_WORLDS]
    c5 = tuple((C5_ROWS, t) for t in range(3))
    out += [
        # key widths: no table is allocated, the route reads ids and num_rows only
        Case("c5-w8-bits32", 8, 3, c5, 300, "fused", seed=1),
        Case("c5-w16-bits33", 16, 3, c5, 300, "multi64", seed=2),
        Case("int32max-w1-bits32", 1, 1, ((INT32_MAX, 0),), 500, "fused", seed=3),
        Case("int32max-w3-bits33", 3, 1, ((INT32_MAX, 0),), 500, "multi64", seed=4),
        Case("int32max-w1-tags202-bits33", 1, 3, ((INT32_MAX, 2), (5000, 0), (INT32_MAX, 2)), 500, "multi64", seed=5),
        Case("w1024-t32-bits46", K_MAX_WORLD, 32, ((INT32_MAX, 31), (5000, 0), (700, 17), (5000, 0)), 40, "multi64",
             seed=6),
        Case("w1024-t2-b5", K_MAX_WORLD, 2, ((5000, 1),), 5, "fused", seed=7),
        # content
        Case("all-invalid", 3, 3, tuple((SIZE_ROWS[t], t) for t in range(3)), 50, "fused", "all_invalid"),
        # ... and in the world-1 multi-launch form, where the head / write passes lay out the slots
        Case("all-invalid-w1-multi", 1, 3, tuple((SIZE_ROWS[t], t) for t in range(3)), K // 3 + 1, "multi32",
             "all_invalid"),
        Case("all-equal", 8, 3, ((5000, 0),), K, "fused", "all_equal"),
        Case("all-distinct", 8, 3, ((100_000, 0),), K, "fused", "all_distinct", seed=8),
        Case("one-row-tables", 8, 2, ((1, 0), (1, 1)), 40, "fused", seed=9),
        Case("empty-tags", 3, 5, ((700, 4), (5000, 1), (700, 4)), 64, "fused", seed=10),
    ]
    return out


CASES = _cases()
CASE_IDS = [c.name for c in CASES]
# the size and key-width cases: the id generator's promise (valid, invalid and
# duplicate ids in one case) holds from three lookups' worth of ids up
GENERATED = [c for c in CASES if c.content == "mixed"]


# --------------------------------------------------------------------------- the contract
class Flat(NamedTuple):
    """Every lookup position l * batch + b of a case: the row it must request
    (-1 for an id outside its table), its tag and its owner."""
    row: np.ndarray
    tag: np.ndarray
    owner: np.ndarray

    @property
    def key(self) -> np.ndarray:  # (owner, tag, row + 1) in one int64; row + 1 = 0 for an invalid id
        return _key(self.owner, self.tag, self.row)


def _owner(row: np.ndarray, world: int) -> np.ndarray:
    return np.where(row >= 0, row % world, world - 1)


def _key(owner, tag, row) -> np.ndarray:
    return (owner.astype(np.int64) << 48) | (tag.astype(np.int64) << 32) | (row.astype(np.int64) + 1)


def flat(case: Case) -> Flat:
    rows, tags = [], []
    for ids, (num_rows, tag) in zip(case.ids(), case.tables):
        r = ids.astype(np.int64)
        rows.append(np.where((r >= 0) & (r < num_rows), r, -1))
        tags.append(np.full(len(r), tag, np.int64))
    row, tag = np.concatenate(rows), np.concatenate(tags)
    return Flat(row, tag, _owner(row, case.world))


def check_requests(case: Case, send, counts, num_requests, idx) -> None:
    """send [>= R, 2], counts [world], num_requests, idx [L, B] against the
    contract of tt_route_requests."""
    send, counts, idx = np.asarray(send, np.int64), np.asarray(counts, np.int64), np.asarray(idx, np.int64)
    R = int(np.asarray(num_requests).reshape(-1)[0])
    W, T = case.world, case.num_tags
    if counts.shape != (W,) or idx.shape != (len(case.tables), case.batch):
        _fail("counts %s / idx %s have the wrong shape", counts.shape, idx.shape)
    if not 1 <= R <= min(case.total, len(send)):
        _fail("num_requests %d outside 1..%d", R, min(case.total, len(send)))
    if int(counts.sum()) != R:
        _fail("counts sum to %d, num_requests is %d", int(counts.sum()), R)
    row, tag = send[:R, 0], send[:R, 1]
    if np.any((tag < 0) | (tag >= T) | (row < -1)):
        _fail("request %d = (%d, %d) is no (row, tag)", _first((tag < 0) | (tag >= T) | (row < -1)),
              *send[_first((tag < 0) | (tag >= T) | (row < -1))])
    pairs = np.unique(send[:R], axis=0)
    if len(pairs) != R:
        _fail("%d requests, %d distinct (row, tag) pairs", R, len(pairs))
    owner = _owner(row, W)
    key = _key(owner, tag, row)
    if np.any(key[1:] <= key[:-1]):
        u = _first(key[1:] <= key[:-1])
        _fail("requests %d, %d = %s, %s are not increasing in (owner, tag, row)", u, u + 1, send[u], send[u + 1])
    want = np.bincount(owner, minlength=W)
    if not np.array_equal(counts, want):
        o = _first(counts != want)
        _fail("counts[%d] = %d, owner %d has %d requests", o, counts[o], o, want[o])
    f = flat(case)
    u = idx.reshape(-1)
    if np.any((u < 0) | (u >= R)):
        _fail("idx[%d] = %d outside 0..%d", _first((u < 0) | (u >= R)), u[_first((u < 0) | (u >= R))], R - 1)
    bad = (row[u] != f.row) | (tag[u] != f.tag)
    if np.any(bad):
        p = _first(bad)
        _fail("lookup %d wants (%d, %d), idx names request %d = %s", p, f.row[p], f.tag[p], u[p], send[u[p]])
    named = np.zeros(R, bool)
    named[u] = True
    if not named.all():
        _fail("request %d = %s is named by no lookup", _first(~named), send[_first(~named)])


def check_ordered(case: Case, order, grp_first, grp_last) -> None:
    """order [L*B], grp_first / grp_last [world*num_tags] against the contract
    of tt_route_requests_ordered."""
    order = np.asarray(order, np.int64)
    gf, gl = np.asarray(grp_first, np.int64), np.asarray(grp_last, np.int64)
    N, G = case.total, case.world * case.num_tags
    if order.shape != (N,) or gf.shape != (G,) or gl.shape != (G,):
        _fail("order %s / grp_first %s / grp_last %s have the wrong shape", order.shape, gf.shape, gl.shape)
    if not np.array_equal(np.sort(order), np.arange(N)):
        _fail("order is no permutation of 0..%d", N - 1)
    f = flat(case)
    ks = f.key[order]
    if np.any(ks[1:] < ks[:-1]):
        p = _first(ks[1:] < ks[:-1])
        _fail("sorted positions %d, %d: the key (owner, tag, row + 1) decreases", p, p + 1)
    tie = (ks[1:] == ks[:-1]) & (order[1:] < order[:-1])
    if np.any(tie):
        p = _first(tie)
        _fail("sorted positions %d, %d: equal keys, lookups %d, %d not in lookup order", p, p + 1, order[p],
              order[p + 1])
    grp = f.owner[order] * case.num_tags + f.tag[order]  # non-decreasing (the key is)
    first = np.searchsorted(grp, np.arange(G), "left")
    last = np.searchsorted(grp, np.arange(G), "right") - 1
    empty = last < first
    first[empty], last[empty] = 0, -1
    if not (np.array_equal(gf, first) and np.array_equal(gl, last)):
        g = _first((gf != first) | (gl != last))
        _fail("group %d (owner %d, tag %d) reads (%d, %d), holds sorted positions (%d, %d)%s", g, g // case.num_tags,
              g % case.num_tags, gf[g], gl[g], first[g], last[g], " (empty)" if empty[g] else "")


class Requests(NamedTuple):
    send: np.ndarray    # [R, 2] int32
    counts: np.ndarray  # [world] int64
    idx: np.ndarray     # [L, B] int32
    start: np.ndarray   # [world + 1]: the first request of each owner


@functools.lru_cache(maxsize=None)
def reference(case: Case) -> Requests:
    """The one answer check_requests admits, built from the distinct keys."""
    f = flat(case)
    keys, inv = np.unique(f.key, return_inverse=True)
    send = np.stack([(keys & 0xFFFFFFFF) - 1, (keys >> 32) & 0xFFFF], 1).astype(np.int32)
    counts = np.bincount(keys >> 48, minlength=case.world).astype(np.int64)
    idx = inv.reshape(len(case.tables), case.batch).astype(np.int32)
    check_requests(case, send, counts, len(keys), idx)
    out = Requests(send, counts, idx, np.concatenate([[0], np.cumsum(counts)]))
    for a in out:
        a.setflags(write=False)
    return out


class Restated(NamedTuple):
    """tests/torch_route.py on a case (CPU tensors; shared, leave unchanged)."""
    send: "torch.Tensor"  # noqa: F821
    counts: "torch.Tensor"  # noqa: F821
    num_requests: "torch.Tensor"  # noqa: F821
    idx: "torch.Tensor"  # noqa: F821
    order: "torch.Tensor"  # noqa: F821
    grp_first: "torch.Tensor"  # noqa: F821
    grp_last: "torch.Tensor"  # noqa: F821

    def padded(self, case: Case, cap: int):
        """(send_padded, idx_padded, dropped requests) of torch_route_pad."""
        import torch
        from torch_route import torch_route_pad

        ov = torch.zeros(1, dtype=torch.int32)
        sp, ip = torch_route_pad(self.send, self.counts, self.idx, case.world, cap, ov)
        return sp, ip, int(ov)


@functools.lru_cache(maxsize=None)
def restated(case: Case) -> Restated:
    import torch
    from torch_route import torch_route_requests

    lookups = [(torch.from_numpy(ids.copy()), rows, tag) for ids, (rows, tag) in zip(case.ids(), case.tables)]
    send, counts, nreq, idx, ordered = torch_route_requests(lookups, case.world, case.num_tags, ordered=True)
    return Restated(send, counts, nreq, idx, *ordered)


def capacities(case: Case) -> List[Tuple[int, bool]]:
    """(cap, overflows) per case: never overflowing (every lookup its own
    slot), exactly full, one request short, and 1.  max(counts) <= total, so
    world * cap stays small at world 1024."""
    m = int(reference(case).counts.max())
    caps = [case.total, m] + ([m - 1] if m - 1 >= 1 else []) + [1]
    return [(c, c < m) for c in sorted(set(caps), reverse=True)]


def dropped(case: Case, cap: int) -> int:
    return int(np.maximum(0, reference(case).counts - cap).sum())


def check_padded(case: Case, cap: int, send_padded, idx_padded, overflow_before: Optional[int] = None,
                 overflow_after: Optional[int] = None) -> None:
    """send_padded [world*cap, 2], idx_padded [L, B] and the overflow word
    before / after the call against the contract of tt_route_pad."""
    sp, ip = np.asarray(send_padded, np.int64), np.asarray(idx_padded, np.int64)
    ref = reference(case)
    W = case.world
    if sp.shape != (W * cap, 2) or ip.shape != ref.idx.shape:
        _fail("send_padded %s / idx_padded %s have the wrong shape", sp.shape, ip.shape)
    o, j = np.divmod(np.arange(W * cap), cap)
    held = j < ref.counts[o]
    want = np.full((W * cap, 2), -1, np.int64)
    want[held] = ref.send[(ref.start[o] + j)[held]]
    if not np.array_equal(sp, want):
        s = _first((sp != want).any(1))
        _fail("slot %d (owner %d, request %d of %d, cap %d) holds %s, contract %s", s, o[s], j[s], ref.counts[o[s]],
              cap, sp[s], want[s])
    u = ref.idx.astype(np.int64)
    own = np.searchsorted(ref.start, u, "right") - 1
    jj = u - ref.start[own]
    slot = np.where(jj < cap, own * cap + jj, -1 - own)
    if not np.array_equal(ip, slot):
        p = _first(ip != slot)
        _fail("lookup %d (request %d of owner %d, cap %d) reads slot %d, contract %d", p, jj.reshape(-1)[p],
              own.reshape(-1)[p], cap, ip.reshape(-1)[p], slot.reshape(-1)[p])
    if overflow_after is not None:
        if int(overflow_after) - int(overflow_before) != dropped(case, cap):
            _fail("overflow went from %d to %d, %d requests were dropped", int(overflow_before), int(overflow_after),
                  dropped(case, cap))


def check_owner(world: int, num_tags: int, recv, tags, rows, table_ids) -> None:
    """tags [n], rows [n], table_ids [num_tags, n] of the requests recv [n, 2]
    against the contract of tt_route_owner."""
    recv, tags, rows, tids = (np.asarray(a, np.int64) for a in (recv, tags, rows, table_ids))
    n = len(recv)
    if tags.shape != (n,) or rows.shape != (n,) or tids.shape != (num_tags, n):
        _fail("tags %s / rows %s / table_ids %s have the wrong shape", tags.shape, rows.shape, tids.shape)
    if not np.array_equal(tags, recv[:, 1]):
        _fail("tags[%d] = %d, the request's tag is %d", _first(tags != recv[:, 1]), tags[_first(tags != recv[:, 1])],
              recv[_first(tags != recv[:, 1]), 1])
    gid = recv[:, 0]
    want = np.where(gid >= 0, gid // world, -1)
    if not np.array_equal(rows, want):
        j = _first(rows != want)
        _fail("rows[%d] = %d, global row %d at world %d is local row %d", j, rows[j], gid[j], world, want[j])
    for t in range(num_tags):
        wt = np.where(recv[:, 1] == t, want, -1)
        if not np.array_equal(tids[t], wt):
            j = _first(tids[t] != wt)
            _fail("table_ids[%d, %d] = %d, contract %d (request %s)", t, j, tids[t, j], wt[j], recv[j])
