"""CPU checks behind tests/test_route_edges_gpu.py.

The GPU tests hold libtt's request routing to the contract checker of
tests/route_ref.py and to the torch restatement of tests/torch_route.py.
That proves something only if (a) the checker accepts a right answer — here
the restatement's, on every case and capacity — (b) it rejects wrong ones —
here one mutation per clause of the contract, each on a case where it
changes the answer — and (c) the cases reach the paths they are listed for:
the path computed from plan_route's bit count equals the declared one, and
all three paths and both sides of kRsMax are populated.  The host side of
the entry points (argument validation: clean errors, no launch) is checked
through the C ABI as tests/test_native_exports.py does.
"""
from collections import Counter

import numpy as np
import pytest
import torch

import route_ref as rr
from pkg import _native
from torch_route import torch_route_owner, torch_route_pad

BY_NAME = {c.name: c for c in rr.CASES}


def _restated(case):
    """torch_route_requests(..., ordered=True) on the case, as numpy arrays
    (views of the shared tensors: copy before changing one)."""
    return [t.numpy() for t in rr.restated(case)]


# --------------------------------------------------------------------------- the case list
def test_case_names_are_unique_and_constants_are_the_kernels():
    assert len(BY_NAME) == len(rr.CASES)
    assert (rr.K_MAX_WORLD, rr.K_MAX_LOOKUPS) == (1024, _native.ROUTE_MAX_LOOKUPS)
    assert rr.K_RS_MAX % 1024 == 0  # the fused kernel stages kRsMax / 1024 lookups per thread
    assert all(len(c.tables) <= rr.K_MAX_LOOKUPS and c.world <= rr.K_MAX_WORLD for c in rr.CASES)
    for c in rr.CASES:  # one row count per tag (what the restatement and the sharded tables assume)
        assert len({t: r for r, t in c.tables}) == len(set(c.tables)), c.name
        assert all(0 <= t < c.num_tags for _, t in c.tables), c.name


def test_declared_paths_equal_the_bit_count():
    for c in rr.CASES:
        assert c.path == rr.route_path(c.total, c.world, c.num_tags, c.max_rows), c.name
    census = Counter(c.path for c in rr.CASES)
    assert census == {"fused": 47, "multi32": 10, "multi64": 4}
    K = rr.K_RS_MAX
    fused_totals = {c.total for c in rr.CASES if c.path == "fused"}
    multi_totals = {c.total for c in rr.CASES if c.path == "multi32"}
    assert {1, 2, 63, 64, 65, 1023, 1024, 1025, K - 1, K} <= fused_totals and max(fused_totals) == K
    assert min(multi_totals) == K + 1 and {3 * (K // 3 + 1), 32 * (K // 32 + 1)} <= multi_totals
    assert max(c.total for c in rr.CASES) == 32 * (K // 32 + 1)
    # the key-width switch from both sides, at the C5 table and at the widest table
    bits = {c.name: (c.end_bit, c.path) for c in rr.CASES}
    assert bits["c5-w8-bits32"] == (32, "fused") and bits["c5-w16-bits33"] == (33, "multi64")
    assert bits["int32max-w1-bits32"] == (32, "fused") and bits["int32max-w3-bits33"] == (33, "multi64")
    assert bits["int32max-w1-tags202-bits33"] == (33, "multi64") and bits["w1024-t32-bits46"] == (46, "multi64")
    assert rr.end_bit(2, 1, rr.INT32_MAX) == 32  # why the 33-bit one-tag case sits at world 3
    assert all(c.total <= K for c in rr.CASES if c.path == "multi64")  # 64-bit keys alone keep them off the fused path


def test_generated_ids_mix_valid_invalid_and_duplicates():
    """Every size and key-width case holds valid ids, invalid ids and at
    least two lookups of one request — from three ids up: with fewer the three
    cannot all hold (1x1 and 1x2 are the only such cases)."""
    small = [c.name for c in rr.GENERATED if c.total < 3]
    assert sorted(small) == sorted(f"1x{b}-w{w}" for b in (1, 2) for w in rr.SIZE_WORLDS)
    for c in rr.GENERATED:
        f = rr.flat(c)
        assert all(x.dtype == np.int32 and x.shape == (c.batch,) for x in c.ids())
        if c.total >= 3:
            assert (f.row >= 0).any() and (f.row < 0).any(), c.name
            assert len(np.unique(f.key)) < c.total, c.name
    big = np.concatenate([x for c in rr.GENERATED if c.max_rows == rr.INT32_MAX for x in c.ids()])
    assert {rr.INT32_MAX, rr.INT32_MIN, rr.INT32_MAX - 1, -1, 0} <= set(big.tolist())


def test_content_cases_are_what_their_names_say():
    ref = {n: rr.reference(BY_NAME[n]) for n in ("all-invalid", "all-equal", "all-distinct", "one-row-tables",
                                                  "empty-tags")}
    for c in (BY_NAME["all-invalid"], BY_NAME["all-invalid-w1-multi"]):
        ans = rr.reference(c)
        assert ans.send.tolist() == [[-1, 0], [-1, 1], [-1, 2]]
        assert ans.counts.tolist() == [0] * (c.world - 1) + [3]
        assert {int(x) for ids in c.ids() for x in ids} == {-1} | {rows for rows, _ in c.tables}
    assert (BY_NAME["all-invalid"].world, BY_NAME["all-invalid-w1-multi"].world) == (3, 1)
    assert ref["all-equal"].send.tolist() == [[4999, 0]] and BY_NAME["all-equal"].total == rr.K_RS_MAX
    assert len(ref["all-distinct"].send) == rr.K_RS_MAX == BY_NAME["all-distinct"].total
    assert set(ref["one-row-tables"].send[:, 0].tolist()) == {-1, 0}
    assert ref["one-row-tables"].counts.tolist() == [2] + [0] * 6 + [2]
    c = BY_NAME["empty-tags"]
    used = {int(o) * c.num_tags + int(t) for o, t in zip(rr.flat(c).owner, rr.flat(c).tag)}
    assert used == {o * 5 + t for o in range(3) for t in (1, 4)}  # nine of the fifteen groups stay empty
    assert [t for _, t in BY_NAME["w1024-t32-bits46"].tables] == [31, 0, 17, 0]  # one tag's lookups not adjacent
    for name in ("w1024-t32-bits46", "w1024-t2-b5"):  # most owners empty
        counts = rr.reference(BY_NAME[name]).counts
        assert counts.shape == (rr.K_MAX_WORLD,) and (counts == 0).sum() >= rr.K_MAX_WORLD - BY_NAME[name].total


def test_capacities_cover_full_short_and_one():
    for c in rr.CASES:
        caps = rr.capacities(c)
        m = int(rr.reference(c).counts.max())
        assert caps[0] == (c.total, False) and (m, False) in caps and caps[-1][0] == 1
        assert all(cap * c.world < 2 ** 22 for cap, _ in caps), c.name
        for cap, over in caps:
            assert over == (rr.dropped(c, cap) > 0)
            if over:  # drops at least one request and keeps at least one
                assert np.minimum(rr.reference(c).counts, cap).sum() >= 1
        if m >= 2:
            assert (m - 1, True) in caps and rr.dropped(c, m - 1) == int((rr.reference(c).counts == m).sum())
    for path in ("fused", "multi32", "multi64"):  # every path drops requests somewhere, at world 1 too
        assert any(over for c in rr.CASES if c.path == path for _, over in rr.capacities(c))
        assert any(over for c in rr.CASES if c.path == path and c.world == 1 for _, over in rr.capacities(c))


# --------------------------------------------------------------------------- the checker accepts the restatement
@pytest.mark.parametrize("case", rr.CASES, ids=rr.CASE_IDS)
def test_checker_accepts_the_torch_restatement(case):
    send, counts, nreq, idx, order, gf, gl = _restated(case)
    rr.check_requests(case, send, counts, nreq, idx)
    rr.check_ordered(case, order, gf, gl)
    ref = rr.reference(case)
    assert np.array_equal(send, ref.send) and np.array_equal(counts, ref.counts) and np.array_equal(idx, ref.idx)
    for cap, over in rr.capacities(case):
        ov = torch.full((1,), 5, dtype=torch.int32)
        sp, ip = torch_route_pad(torch.from_numpy(send), torch.from_numpy(counts), torch.from_numpy(idx), case.world,
                                 cap, ov)
        rr.check_padded(case, cap, sp.numpy(), ip.numpy(), 5, int(ov))
        assert (int(ov) > 5) == over
        tags, rows, tids = torch_route_owner(sp, case.world, case.num_tags)
        rr.check_owner(case.world, case.num_tags, sp.numpy(), tags.numpy(), rows.numpy(), tids.numpy())


# --------------------------------------------------------------------------- the checker bites
def _answer(name):
    case = BY_NAME[name]
    return case, [a.copy() for a in _restated(case)]


def _padded(case, cap, send, counts, idx):
    ov = torch.zeros(1, dtype=torch.int32)
    sp, ip = torch_route_pad(torch.from_numpy(send), torch.from_numpy(counts), torch.from_numpy(idx), case.world, cap, ov)
    return sp.numpy().copy(), ip.numpy().copy(), int(ov)


def _rejected(check, right, wrong):
    """`check(*right)` passes, `wrong` differs from `right`, `check(*wrong)` raises."""
    check(*right)
    assert any(not np.array_equal(a, b) for a, b in zip(right, wrong)), "the mutation changed nothing"
    with pytest.raises(rr.RouteMismatch):
        check(*wrong)


MUTATION_CASE = "empty-tags"  # world 3, five tags of which two are used: duplicates, invalid ids, empty groups


def test_checker_rejects_swapped_requests():
    case, (send, counts, nreq, idx, *_) = _answer(MUTATION_CASE)
    bad = send.copy()
    bad[[4, 5]] = bad[[5, 4]]
    _rejected(lambda s, i: rr.check_requests(case, s, counts, nreq, i), (send, idx), (bad, idx))
    # ... and with idx following the swap, so that only the order is wrong
    follow = idx.copy()
    follow[idx == 4], follow[idx == 5] = 5, 4
    _rejected(lambda s, i: rr.check_requests(case, s, counts, nreq, i), (send, idx), (bad, follow))


def test_checker_rejects_a_duplicated_request():
    case, (send, counts, nreq, idx, *_) = _answer(MUTATION_CASE)
    R = int(nreq[0])
    u = 2
    owner = int(np.searchsorted(np.cumsum(counts), u, "right"))
    dup = np.concatenate([send[:u + 1], send[u:R], send[R:-1]])  # request u twice, everything after it one later
    c2 = counts.copy()
    c2[owner] += 1
    shifted = np.where(idx > u, idx + 1, idx).astype(np.int32)
    _rejected(lambda s, c, n, i: rr.check_requests(case, s, c, n, i), (send, counts, nreq, idx),
              (dup, c2, np.array([R + 1], np.int32), shifted))


def test_checker_rejects_a_count_moved_between_owners():
    case, (send, counts, nreq, idx, *_) = _answer(MUTATION_CASE)
    bad = counts.copy()
    bad[0] -= 1
    bad[1] += 1
    _rejected(lambda c: rr.check_requests(case, send, c, nreq, idx), (counts,), (bad,))


def test_checker_rejects_an_idx_naming_the_neighbour():
    case, (send, counts, nreq, idx, *_) = _answer(MUTATION_CASE)
    for step in (1, -1):
        bad = idx.copy()
        bad[1, 7] += step if 0 <= bad[1, 7] + step < int(nreq[0]) else -step
        _rejected(lambda i: rr.check_requests(case, send, counts, nreq, i), (idx,), (bad,))


def test_checker_rejects_an_unnamed_request():
    """A request no lookup names: the all-equal case with a second request."""
    case, (send, counts, nreq, idx, *_) = _answer("all-equal")
    extra = np.array([[4999, 0], [4991, 1]], np.int32)  # same owner (4999 % 8 == 4991 % 8), a later tag
    c2 = counts.copy()
    c2[4999 % 8] += 1
    _rejected(lambda s, c, n: rr.check_requests(case, s, c, n, idx), (send, counts, nreq),
              (extra, c2, np.array([2], np.int32)))


def test_checker_rejects_an_unstable_order():
    case, (*_, order, gf, gl) = _answer(MUTATION_CASE)
    key = rr.flat(case).key[order]
    p = int(np.flatnonzero(key[1:] == key[:-1])[0])  # two lookups of one request
    bad = order.copy()
    bad[[p, p + 1]] = bad[[p + 1, p]]
    _rejected(lambda o: rr.check_ordered(case, o, gf, gl), (order,), (bad,))
    # ... and an order that is not sorted at all
    q = int(np.flatnonzero(key[1:] != key[:-1])[0])
    bad = order.copy()
    bad[[q, q + 1]] = bad[[q + 1, q]]
    _rejected(lambda o: rr.check_ordered(case, o, gf, gl), (order,), (bad,))


def test_checker_rejects_wrong_group_bounds():
    case, (*_, order, gf, gl) = _answer(MUTATION_CASE)
    full = int(np.flatnonzero(gl >= 0)[1])
    empty = int(np.flatnonzero(gl < 0)[0])
    assert gf[empty] == 0 and gl[empty] == -1
    low = gl.copy()
    low[full] -= 1
    _rejected(lambda f, l: rr.check_ordered(case, order, f, l), (gf, gl), (gf, low))
    zero = gl.copy()
    zero[empty] = 0  # an empty group reading (0, 0): one lookup at sorted position 0
    _rejected(lambda f, l: rr.check_ordered(case, order, f, l), (gf, gl), (gf, zero))
    late = gf.copy()
    late[full] += 1
    _rejected(lambda f, l: rr.check_ordered(case, order, f, l), (gf, gl), (late, gl))


def test_checker_rejects_wrong_slots_sentinels_and_overflow():
    case, (send, counts, nreq, idx, *_) = _answer(MUTATION_CASE)
    roomy, tight = case.total, int(counts.max()) - 1
    sp, ip, ov = _padded(case, roomy, send, counts, idx)
    assert ov == 0
    filler = int(np.flatnonzero(sp[:, 1] < 0)[0])
    bad = sp.copy()
    bad[filler] = (0, -1)
    _rejected(lambda s, i: rr.check_padded(case, roomy, s, i, 5, 5), (sp, ip), (bad, ip))
    with pytest.raises(rr.RouteMismatch):
        rr.check_padded(case, roomy, sp, ip, 5, 6)  # nothing dropped: overflow must stay
    sp, ip, ov = _padded(case, tight, send, counts, idx)
    assert ov == rr.dropped(case, tight) > 0
    rr.check_padded(case, tight, sp, ip, 5, 5 + ov)
    rr.check_padded(case, tight, sp, ip)  # no overflow word: nothing to check there
    for off in (-1, 1):
        with pytest.raises(rr.RouteMismatch):
            rr.check_padded(case, tight, sp, ip, 5, 5 + ov + off)
    lost = np.argwhere(ip < 0)[0]
    bad = ip.copy()
    bad[tuple(lost)] -= 1  # -1 - (owner + 1)
    _rejected(lambda s, i: rr.check_padded(case, tight, s, i, 0, ov), (sp, ip), (sp, bad))
    kept = sp.copy()
    last = tight - 1  # owner 0's last kept slot holding the request after it
    start = np.concatenate([[0], np.cumsum(counts)])
    full_owner = int(np.argmax(counts))
    kept[full_owner * tight + last] = send[start[full_owner] + last + 1]
    _rejected(lambda s, i: rr.check_padded(case, tight, s, i, 0, ov), (sp, ip), (kept, ip))


def test_checker_rejects_an_undivided_owner_row():
    case, (send, counts, nreq, idx, *_) = _answer(MUTATION_CASE)
    sp, _, _ = _padded(case, case.total, send, counts, idx)
    tags, rows, tids = (t.numpy().copy() for t in torch_route_owner(torch.from_numpy(sp), case.world, case.num_tags))
    j = int(np.flatnonzero(sp[:, 0] >= case.world)[0])
    bad_rows, bad_tids = rows.copy(), tids.copy()
    bad_rows[j] = sp[j, 0]
    bad_tids[sp[j, 1], j] = sp[j, 0]
    check = lambda r, t: rr.check_owner(case.world, case.num_tags, sp, tags, r, t)  # noqa: E731
    _rejected(check, (rows, tids), (bad_rows, tids))
    _rejected(check, (rows, tids), (rows, bad_tids))
    filler = int(np.flatnonzero(sp[:, 1] < 0)[0])
    bad_tids = tids.copy()
    bad_tids[0, filler] = 0  # a filler slot gives -1 in every table's row list
    _rejected(check, (rows, tids), (rows, bad_tids))


# --------------------------------------------------------------------------- host validation
FAKE = 4096  # a non-NULL, 16-byte aligned address no call below dereferences
BIG = 1 << 40


def _lookups(n=1, rows=100, tag=0, ids=FAKE):
    arr = (_native.RouteLookup * max(n, 1))()
    for x in arr:
        x.ids, x.num_rows, x.tag = ids, rows, tag
    return arr


def _ordered(lk=None, n=1, batch=4, world=2, num_tags=1, grp=(FAKE, FAKE), ws=FAKE, ws_bytes=BIG):
    lk = _lookups(n) if lk is None else lk
    return _native.lib().tt_route_requests_ordered(lk, n, batch, world, num_tags, FAKE, FAKE, FAKE, FAKE, FAKE,
                                                   grp[0], grp[1], ws, ws_bytes, None)


def _requests(lk=None, n=1, batch=4, world=2, num_tags=1, grp=None, ws=FAKE, ws_bytes=BIG):
    lk = _lookups(n) if lk is None else lk
    return _native.lib().tt_route_requests(lk, n, batch, world, num_tags, FAKE, FAKE, FAKE, FAKE, ws, ws_bytes, None)


def _fixed(lk=None, n=1, batch=4, world=2, num_tags=1, grp=(FAKE, FAKE), ws=FAKE, ws_bytes=BIG, cap=4,
           owner=(None, None, None)):
    lk = _lookups(n) if lk is None else lk
    return _native.lib().tt_route_fixed(lk, n, batch, world, num_tags, cap, FAKE, FAKE, FAKE, FAKE, FAKE, grp[0],
                                        grp[1], owner[0], owner[1], owner[2], ws, ws_bytes, None)


def _refused(rc, code=_native.TT_ERR_BAD_ARG, *words):
    """A host-side refusal: its own status (a launch on a host without a GPU
    would report TT_ERR_HIP instead) and an error text naming the route."""
    assert rc == code
    with pytest.raises(_native.TTError) as e:
        _native.check(rc)
    msg = str(e.value)
    assert "route" in msg and all(w in msg for w in words), msg


ENTRIES = [_ordered, _requests, _fixed]
ENTRY_IDS = ["requests_ordered", "requests", "fixed"]


@pytest.mark.parametrize("entry", ENTRIES, ids=ENTRY_IDS)
def test_route_entries_refuse_bad_shapes(entry):
    _refused(entry(world=0), _native.TT_ERR_BAD_ARG, "world 0")
    _refused(entry(world=rr.K_MAX_WORLD + 1), _native.TT_ERR_BAD_ARG, f"world {rr.K_MAX_WORLD + 1}")
    _refused(entry(n=0), _native.TT_ERR_BAD_ARG, "lookups", "got 0")
    _refused(entry(n=rr.K_MAX_LOOKUPS + 1), _native.TT_ERR_BAD_ARG, f"1..{rr.K_MAX_LOOKUPS} lookups")
    _refused(entry(batch=0), _native.TT_ERR_BAD_ARG, "empty batch")
    _refused(entry(num_tags=0), _native.TT_ERR_BAD_ARG, "num_tags")
    _refused(entry(_lookups(1, tag=3), num_tags=3), _native.TT_ERR_BAD_ARG, "lookup 0 tag")
    _refused(entry(_lookups(1, tag=-1), num_tags=3), _native.TT_ERR_BAD_ARG, "lookup 0 tag")
    second = _lookups(2)
    second[1].tag = 1
    _refused(entry(second, n=2), _native.TT_ERR_BAD_ARG, "lookup 1 tag")
    _refused(entry(_lookups(1, rows=0)), _native.TT_ERR_BAD_ARG, "lookup 0", "num_rows")
    _refused(entry(_lookups(1, rows=2 ** 31)), _native.TT_ERR_BAD_ARG, "lookup 0", "num_rows")
    _refused(entry(_lookups(1, ids=None)), _native.TT_ERR_BAD_ARG, "lookup 0")
    if entry is not _requests:
        _refused(entry(grp=(FAKE, None)), _native.TT_ERR_BAD_ARG, "grp_first / grp_last")
        _refused(entry(grp=(None, FAKE)), _native.TT_ERR_BAD_ARG, "grp_first / grp_last")
    # a table of 2^31 - 1 rows is the widest one the route takes: refused below for its workspace, not its rows


@pytest.mark.parametrize("entry", ENTRIES, ids=ENTRY_IDS)
def test_route_entries_refuse_a_small_workspace_without_a_launch(entry):
    """The multi-launch forms (more than kRsMax lookups, or keys wider than 32
    bits at any size; tt_route_requests* always) need the workspace
    tt_route_*_workspace_size states, and say so before anything is launched."""
    L = _native.lib()
    size = L.tt_route_workspace_size if entry is not _fixed else L.tt_route_fixed_workspace_size
    for rows, batch, world, path in ((5000, rr.K_RS_MAX + 1, 1, "multi32"), (5000, rr.K_RS_MAX + 1, 3, "multi32"),
                                     (rr.INT32_MAX, 4, 3, "multi64"), (rr.INT32_MAX, 4, 1, "fused")):
        lk = _lookups(1, rows=rows)
        assert rr.route_path(batch, world, 1, rows) == path
        if entry is _fixed and path == "fused":
            continue  # one workgroup, no workspace: nothing to refuse
        # the sort's keys alone take 16 bytes per lookup: half of that can never do (the stated size has slack,
        # so one byte less than it may still be enough, and these pointers must never reach a launch)
        assert size(1, batch, world, lk[0].num_rows, 1) >= batch * 24
        _refused(entry(lk, batch=batch, world=world, ws_bytes=batch * 8), _native.TT_ERR_WORKSPACE, "workspace", "required")
        _refused(entry(lk, batch=batch, world=world, ws=None), _native.TT_ERR_WORKSPACE, "workspace")


def test_route_fixed_refuses_bad_capacities_and_owner_views():
    _refused(_fixed(cap=0), _native.TT_ERR_BAD_ARG, "tt_route_fixed", "cap")
    _refused(_fixed(cap=-3), _native.TT_ERR_BAD_ARG, "tt_route_fixed", "cap")
    _refused(_fixed(world=2, cap=2 ** 30), _native.TT_ERR_BAD_ARG, "tt_route_fixed", "cap")
    _refused(_fixed(world=rr.K_MAX_WORLD, cap=2 ** 21), _native.TT_ERR_BAD_ARG, "tt_route_fixed", "cap")
    _refused(_fixed(world=2, owner=(FAKE, FAKE, FAKE)), _native.TT_ERR_BAD_ARG, "tt_route_fixed", "owner view", "world 2")
    for owner in ((FAKE, None, None), (FAKE, FAKE, None), (None, FAKE, FAKE)):
        _refused(_fixed(world=1, owner=owner), _native.TT_ERR_BAD_ARG, "tt_route_fixed", "all or none")
    L = _native.lib()
    rc = L.tt_route_fixed(None, 1, 4, 2, 1, 4, FAKE, FAKE, FAKE, None, None, None, None, None, None, None, FAKE, BIG,
                          None)
    _refused(rc, _native.TT_ERR_BAD_ARG, "tt_route_fixed", "NULL")
    rc = L.tt_route_fixed(_lookups(), 1, 4, 2, 1, 4, FAKE, FAKE, None, None, None, None, None, None, None, None, FAKE,
                          BIG, None)
    _refused(rc, _native.TT_ERR_BAD_ARG, "tt_route_fixed", "NULL")


def test_route_pad_refuses_bad_arguments():
    L = _native.lib()

    def pad(send=FAKE, n=8, world=2, cap=4, out=FAKE):
        return L.tt_route_pad(send, FAKE, FAKE, n, world, cap, out, FAKE, None, None)

    _refused(pad(world=0), _native.TT_ERR_BAD_ARG, "tt_route_pad", "world 0")
    _refused(pad(world=rr.K_MAX_WORLD + 1), _native.TT_ERR_BAD_ARG, "tt_route_pad", f"world {rr.K_MAX_WORLD + 1}")
    _refused(pad(cap=0), _native.TT_ERR_BAD_ARG, "tt_route_pad", "cap 0")
    _refused(pad(n=0), _native.TT_ERR_BAD_ARG, "tt_route_pad", "lookups 0")
    _refused(pad(world=2, cap=2 ** 30), _native.TT_ERR_BAD_ARG, "tt_route_pad", "int32")
    _refused(pad(send=None), _native.TT_ERR_BAD_ARG, "tt_route_pad", "NULL")
    _refused(pad(out=None), _native.TT_ERR_BAD_ARG, "tt_route_pad", "NULL")


def test_route_owner_refuses_bad_arguments():
    L = _native.lib()

    def own(recv=FAKE, n=8, world=2, num_tags=3, tids=FAKE):
        return L.tt_route_owner(recv, n, world, num_tags, FAKE, FAKE, tids, None)

    _refused(own(n=-1), _native.TT_ERR_BAD_ARG, "tt_route_owner")
    _refused(own(world=0), _native.TT_ERR_BAD_ARG, "tt_route_owner")
    _refused(own(num_tags=0), _native.TT_ERR_BAD_ARG, "tt_route_owner")
    _refused(own(recv=None), _native.TT_ERR_BAD_ARG, "tt_route_owner", "NULL")
    _refused(own(tids=None), _native.TT_ERR_BAD_ARG, "tt_route_owner", "NULL")
    assert own(recv=None, n=0) == _native.TT_OK  # no requests received: nothing to do, nothing read


def test_route_workspace_queries():
    L = _native.lib()
    for size in (L.tt_route_workspace_size, L.tt_route_fixed_workspace_size):
        assert size(0, 4, 1, 100, 1) == 0 and size(1, 0, 1, 100, 1) == 0
        assert size(1, 4, 0, 100, 1) == 0 and size(1, 4, 1, 100, 0) == 0
    for args in ((3, 4096, 8, rr.C5_ROWS, 3), (3, 300, 16, rr.C5_ROWS, 3), (1, 1, 1, 1, 1)):
        base, fixed = L.tt_route_workspace_size(*args), L.tt_route_fixed_workspace_size(*args)
        total = args[0] * args[1]
        assert base >= total * 24  # keys in and out (8 bytes each), values in and out
        assert fixed >= base + total * 12 + 4  # + the compact send, idx and the request count
