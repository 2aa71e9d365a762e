"""libtt's request routing against its contract, at the edges.

Every case of tests/route_ref.py (sizes on both sides of the one-workgroup
limit kRsMax, keys of 32, 33 and 46 bits, world 1 to 1024, all ids invalid /
equal / distinct, one-row tables, unused tags, non-adjacent lookups of one
tag), at the capacities route_ref.capacities gives (never overflowing,
exactly full, one request short, 1):

  * the composed calls tt_route_requests_ordered -> tt_route_pad ->
    tt_route_owner (always the device sort, 32- or 64-bit keys), and
  * tt_route_fixed (the one-workgroup kernel where the case says `fused`,
    else the multi-launch forms: at world 1 the head / write passes lay the
    slots out themselves, otherwise tt_route_pad's kernel follows)

are held to the contract checker (include/tt.h restated, exact) and to the
torch restatement of tests/torch_route.py, element for element.  Which path a
case takes follows from its size and key width alone (TT_ROUTE_FUSED is read
once per process and left alone); tests/test_route_ref_host.py checks that the
declared paths are the computed ones and that the checker rejects wrong
answers.  The round trip at the end ties the slots to what a lookup finally
reads from row-sharded tables.
"""
import functools

import numpy as np
import pytest
import torch

import route_ref as rr
from pkg.modelling import hip_ops
from torch_route import torch_route_owner

pytestmark = pytest.mark.gpu

PRESET = 5  # what the overflow word holds before a call: the route adds to it


@functools.lru_cache(maxsize=None)
def _lookups(case, cuda):
    return [(torch.from_numpy(ids.copy()).to(cuda), rows, tag) for ids, (rows, tag) in zip(case.ids(), case.tables)]


def _host(*tensors):
    return [t.cpu() for t in tensors]


def _same(got, want, what):
    assert got.dtype == want.dtype and torch.equal(got, want), what


def _owner_views(send_padded, world, num_tags, cap):
    """tt_route_owner on each owner's `cap` slots, fillers included: (tags,
    rows, table_ids) over all slots, fetched once."""
    parts = [hip_ops.route_owner(send_padded[o * cap:(o + 1) * cap], world, num_tags) for o in range(world)]
    return _host(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts], 1))


def _check_drops(case, cap, over, idx_padded, overflow):
    """Non-vacuity: an overflowing capacity drops and keeps requests, and the
    lookups show it; another leaves the overflow word as it was."""
    n = rr.dropped(case, cap)
    assert (n > 0) == over
    if over:
        assert int((idx_padded < 0).sum()) >= n and bool((idx_padded >= 0).any())
    if overflow is not None:
        assert int(overflow) == PRESET + n


@pytest.mark.parametrize("case", rr.CASES, ids=rr.CASE_IDS)
def test_composed_route_meets_the_contract(cuda, case):
    W, T = case.world, case.num_tags
    lookups = _lookups(case, cuda)
    d_send, d_counts, d_nreq, d_idx, d_ord = hip_ops.route_requests(lookups, W, T, ordered=True)
    send, counts, nreq, idx, order, gf, gl = _host(d_send, d_counts, d_nreq, d_idx, *d_ord)
    rr.check_requests(case, send.numpy(), counts.numpy(), nreq.numpy(), idx.numpy())
    rr.check_ordered(case, order.numpy(), gf.numpy(), gl.numpy())
    ref = rr.restated(case)
    R = int(nreq)
    for got, want, what in ((send[:R], ref.send, "send"), (counts, ref.counts, "counts"), (nreq, ref.num_requests, "R"),
                            (idx, ref.idx, "idx"), (order, ref.order, "order"), (gf, ref.grp_first, "grp_first"),
                            (gl, ref.grp_last, "grp_last")):
        _same(got, want, what)
    plain = _host(*hip_ops.route_requests(lookups, W, T))  # without the ordered outputs: the same requests
    for got, want, what in zip(plain, (send, counts, nreq, idx), ("send", "counts", "R", "idx")):
        _same(got[:R] if what == "send" else got, want[:R] if what == "send" else want, what)
    for cap, over in rr.capacities(case):
        want_sp, want_ip, _ = ref.padded(case, cap)
        for preset in (PRESET, None):
            ov = None if preset is None else torch.full((1,), preset, dtype=torch.int32, device=cuda)
            d_sp, d_ip = hip_ops.route_pad(d_send, d_counts, d_idx, W, cap, ov)
            sp, ip = _host(d_sp, d_ip)
            after = None if ov is None else int(ov.item())
            rr.check_padded(case, cap, sp.numpy(), ip.numpy(), preset, after)
            _check_drops(case, cap, over, ip.numpy(), after)
            _same(sp, want_sp, f"send_padded cap {cap}")
            _same(ip, want_ip, f"idx_padded cap {cap}")
        tags, rows, tids = _owner_views(d_sp, W, T, cap)
        for o in range(W):
            s = slice(o * cap, (o + 1) * cap)
            rr.check_owner(W, T, sp[s].numpy(), tags[s].numpy(), rows[s].numpy(), tids[:, s].numpy())
        for got, want, what in zip((tags, rows, tids), torch_route_owner(sp, W, T), ("tags", "rows", "table_ids")):
            _same(got, want, f"owner {what} cap {cap}")


@pytest.mark.parametrize("case", rr.CASES, ids=rr.CASE_IDS)
def test_route_fixed_meets_the_contract(cuda, case):
    W, T = case.world, case.num_tags
    lookups = _lookups(case, cuda)
    ref = rr.restated(case)
    oracle = rr.reference(case)
    for cap, over in rr.capacities(case):
        ov = torch.full((1,), PRESET, dtype=torch.int32, device=cuda)
        d_sp, d_ip, d_counts, d_ord, d_own = hip_ops.route_fixed(lookups, W, T, cap, ov, ordered=True, owner=W == 1)
        sp, ip, counts, order, gf, gl, ov = _host(d_sp, d_ip, d_counts, *d_ord, ov)
        what = f"cap {cap}"
        rr.check_padded(case, cap, sp.numpy(), ip.numpy(), PRESET, int(ov))
        rr.check_ordered(case, order.numpy(), gf.numpy(), gl.numpy())
        assert np.array_equal(counts.numpy(), oracle.counts) and counts.dtype == torch.int64, what
        _check_drops(case, cap, over, ip.numpy(), int(ov))
        want_sp, want_ip, _ = ref.padded(case, cap)
        for got, want, name in ((sp, want_sp, "send_padded"), (ip, want_ip, "idx_padded"), (counts, ref.counts, "counts"),
                                (order, ref.order, "order"), (gf, ref.grp_first, "grp_first"),
                                (gl, ref.grp_last, "grp_last")):
            _same(got, want, f"{name} {what}")
        if W == 1:  # the slots are the one owner's requests
            tags, rows, tids = _host(*d_own)
            rr.check_owner(1, T, sp.numpy(), tags.numpy(), rows.numpy(), tids.numpy())
            for got, want, name in zip((tags, rows, tids), torch_route_owner(sp, 1, T), ("tags", "rows", "table_ids")):
                _same(got, want, f"owner {name} {what}")
        else:
            assert d_own is None
        # none of the optional outputs asked for: the others do not change
        b_sp, b_ip, b_counts, b_ord, b_own = hip_ops.route_fixed(lookups, W, T, cap)
        assert b_ord is None and b_own is None
        for got, want, name in zip(_host(b_sp, b_ip, b_counts), (sp, ip, counts), ("send_padded", "idx_padded", "counts")):
            _same(got, want, f"{name} {what}, bare call")


TRIP_TABLES = ((5000, 0), (700, 1), (5000, 0))
TRIP_DIM = 4


@pytest.mark.parametrize("overflowing", [False, True], ids=["roomy", "overflowing"])
@pytest.mark.parametrize("world", rr.SIZE_WORLDS)
def test_round_trip_reads_the_looked_up_rows(cuda, world, overflowing):
    """Route, answer as each owner would from its shard (rows o::world), read
    back through idx_padded: a kept lookup of a valid id reads its table row
    bit for bit, an invalid or dropped one a zero row."""
    case = rr.Case(f"trip-w{world}", world, 2, TRIP_TABLES, 97, "fused", seed=50 + world)
    m = int(rr.reference(case).counts.max())
    cap = m - 1 if overflowing else case.total
    rng = np.random.default_rng(world)
    tables = [rng.standard_normal((rows, TRIP_DIM)).astype(np.float32) for rows in (5000, 700)]
    assert all((t != 0).all() for t in tables)
    ov = torch.zeros(1, dtype=torch.int32, device=cuda)
    sp, ip, _, _, _ = hip_ops.route_fixed(_lookups(case, cuda), world, 2, cap, ov)
    answers = []
    for o in range(world):
        shards = [torch.as_tensor(np.ascontiguousarray(t[o::world]), device=cuda) for t in tables]
        tags, rows, _ = hip_ops.route_owner(sp[o * cap:(o + 1) * cap], world, 2)
        out = torch.full((cap, TRIP_DIM), float("nan"), device=cuda)
        answers.append(hip_ops.gather_tagged(shards, tags, rows, out))
    answers, slot, ov = torch.cat(answers).cpu().numpy(), ip.cpu().numpy(), ov.item()
    assert not np.isnan(answers).any()  # every slot answered, fillers with zeros
    kept = slot >= 0
    got = np.zeros(slot.shape + (TRIP_DIM,), np.float32)
    got[kept] = answers[slot[kept]]
    want = np.zeros_like(got)
    valid = np.zeros(slot.shape, bool)
    for l, (ids, (rows, tag)) in enumerate(zip(case.ids(), case.tables)):
        valid[l] = (ids >= 0) & (ids < rows)
        want[l, valid[l] & kept[l]] = tables[tag][ids[valid[l] & kept[l]]]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (valid & kept).sum() > case.total // 4 and (~valid & kept).any()
    assert int(ov) == rr.dropped(case, cap) and (int(ov) > 0) == overflowing
    assert bool((valid & ~kept).any()) == overflowing
