"""CPU: the exact top-k with per-query exclusions, everything but the kernel —
the numpy restatement (tests/topk_exclude_ref.py), tt_topk_exclude's host
validation, the host planning (pkg.modelling.indices.exclusions), the sharded
orchestration over gloo with the CPU oracle injected, and IndexRecall's
forwarding."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import topk_exclude_ref as ref
from pkg import _native
from pkg.modelling.indices import exclusions as excl

PAD = 0x7FFFFFFF


# --------------------------------------------------------------------------- the helper
def test_helper_agrees_with_a_python_loop():
    s = np.array([[9, 7, 7, 7, 3, 1], [5, 4, 3, -np.inf, -np.inf, -np.inf]], np.float32)
    i = np.array([[4, 1, 2, 8, 0, 6], [3, 2, 9, 7, PAD, PAD]], np.int32)
    rows = [[2, 6, 2, 100, -1, PAD], [3, 2, 9, 7]]
    off, flat = ref.csr_of(rows)
    for k_out in (1, 3, 6):
        os_, oi, kept, surv = ref.exclude_lists(s, i, off, flat, k_out)
        for q in range(2):
            want = []
            for j in range(6):  # the brute-force loop: keep unless some exclusion equals the index
                hit = False
                for v in rows[q]:
                    if v >= 0 and v != PAD and v == i[q, j]:
                        hit = True
                if not hit:
                    want.append((s[q, j], i[q, j]))
            assert surv[q] == len(want)
            want = want[:k_out]
            assert kept[q] == len(want)
            want += [(-np.inf, PAD)] * (k_out - len(want))
            assert [w[1] for w in want] == oi[q].tolist()
            assert np.array_equal(np.array([w[0] for w in want], np.float32), os_[q])
    # row 1 keeps only its two input padding entries (never removed)
    _, oi, kept, _ = ref.exclude_lists(s, i, off, flat, 6)
    assert kept.tolist() == [4, 2] and oi[1].tolist() == [PAD] * 6


def test_helper_filtered_topk_tiny():
    sc = np.array([[1, 5, 5, 2, 0], [0, 0, 0, 0, 0]], np.float32)
    s, i = ref.filtered_topk(sc, [[1], [0, 2, 99, -3]], 3)
    assert i.tolist() == [[2, 3, 0], [1, 3, 4]] and s.tolist() == [[5, 2, 1], [0, 0, 0]]
    s, i = ref.filtered_topk(sc, [[0, 1, 2, 3], []], 3)
    assert i[0].tolist() == [4, PAD, PAD] and s[0].tolist() == [0, -np.inf, -np.inf]


# --------------------------------------------------------------------------- C ABI validation
def test_topk_exclude_host_validation():
    """Every call is rejected (or returns) on the host: no kernel is launched,
    so fake non-NULL pointers are never dereferenced."""
    lib = _native.lib()
    p = 64  # a non-NULL "pointer"
    def ok(**kw):
        return dict(dict(scores=p, idx=p, n=3, k_in=8, k_out=4, off=p, eidx=p, os=p, oi=p, kept=None), **kw)

    def call(a):
        return lib.tt_topk_exclude(a["scores"], a["idx"], a["n"], a["k_in"], a["k_out"], a["off"], a["eidx"], a["os"],
                                   a["oi"], a["kept"], None)

    for name in ("scores", "idx", "off", "os", "oi"):
        assert call(ok(**{name: None})) == _native.TT_ERR_BAD_ARG, name
        assert "tt_topk_exclude" in lib.tt_last_error().decode()
    assert call(ok(k_out=9)) == _native.TT_ERR_BAD_ARG        # k_out > k_in
    assert call(ok(k_in=4097, k_out=4)) == _native.TT_ERR_BAD_ARG
    assert "4096" in lib.tt_last_error().decode()
    assert call(ok(k_out=0)) == _native.TT_ERR_BAD_ARG
    assert call(ok(k_in=0, k_out=0)) == _native.TT_ERR_BAD_ARG
    assert call(ok(n=-1)) == _native.TT_ERR_BAD_ARG
    assert call(ok(n=0)) == _native.TT_OK
    assert call(ok(n=0, scores=None, idx=None, off=None, eidx=None, os=None, oi=None)) == _native.TT_OK
    with pytest.raises(_native.TTError):
        _native.check(call(ok(k_out=9)))


def test_hip_ops_topk_exclude_argument_checks():
    from pkg.modelling import hip_ops

    s, i = torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int32)
    off, e = torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        hip_ops.topk_exclude(s, i, off, e, 2)  # CPU tensors: libtt has no CPU path


# --------------------------------------------------------------------------- as_csr
def test_as_csr_forms_agree():
    rows = [[5, 2, 2], [], [7], [], [1, 0, 3, 9]]
    padded = torch.full((5, 4), -1, dtype=torch.int64)
    for q, r in enumerate(rows):
        padded[q, :len(r)] = torch.tensor(r, dtype=torch.int64)
    off_np, flat_np = ref.csr_of(rows)
    forms = [padded, padded.numpy().astype(np.int32), rows, [np.asarray(r, np.int64) for r in rows],
             (torch.from_numpy(off_np), torch.from_numpy(flat_np)), (off_np, flat_np)]
    for f in forms:
        off, idx, counts = excl.as_csr(f, 5)
        assert off.dtype == torch.int64 and idx.dtype == torch.int32
        assert off.tolist() == [0, 3, 3, 4, 4, 8] and idx.tolist() == [5, 2, 2, 7, 1, 0, 3, 9]
        assert counts.tolist() == [3, 0, 1, 0, 4]
    off, idx, counts = excl.as_csr([[], []], 2)  # only empty rows
    assert off.tolist() == [0, 0, 0] and idx.numel() == 0 and counts.tolist() == [0, 0]
    off, idx, counts = excl.as_csr(torch.full((2, 3), -7), 2)
    assert off.tolist() == [0, 0, 0] and idx.numel() == 0
    off, idx, counts = excl.as_csr([], 0)
    assert off.tolist() == [0] and counts.numel() == 0
    with pytest.raises(ValueError):
        excl.as_csr(rows, 4)
    with pytest.raises(ValueError):
        excl.as_csr((np.array([0, 2, 1, 3]), np.arange(3)), 3)  # decreasing offsets
    with pytest.raises(ValueError):
        excl.as_csr((np.array([0, 2, 5]), np.arange(3)), 2)  # runs past idx
    with pytest.raises(TypeError):
        excl.as_csr(torch.zeros(2, 2), 2)


def test_take_rows_and_drop_negative():
    off, idx, _ = excl.as_csr([[5, 2], [], [7], [1, 0, 3]], 4)
    o, i = excl.take_rows(off, idx, torch.tensor([3, 0, 1]))
    assert o.tolist() == [0, 3, 5, 5] and i.tolist() == [1, 0, 3, 5, 2]
    o, i = excl.take_rows(off, idx, torch.tensor([1]), 0)
    assert o.tolist() == [0, 0] and i.numel() == 0
    o, i = excl.drop_negative(torch.tensor([0, 2, 2, 5]), torch.tensor([-1, 4, 3, -1, -1], dtype=torch.int32))
    assert o.tolist() == [0, 1, 1, 2] and i.tolist() == [4, 3]


# --------------------------------------------------------------------------- plan_classes
def test_plan_classes_bounds_and_k():
    counts = torch.tensor([0, 1, 16, 17, 64, 65, 256, 257, 1024, 1025, 0, 3000, 5])
    classes = excl.plan_classes(counts, 100, 10 ** 6)
    want = {0: ([0, 10], 100), 16: ([1, 2, 12], 116), 64: ([3, 4], 164), 256: ([5, 6], 356), 1024: ([7, 8], 1124),
            3000: ([9, 11], 3100)}
    assert len(classes) == 6
    for c in classes:
        rows, kp = want[c.count]
        assert c.rows.tolist() == rows and c.k_search == kp and c.total == int(counts[rows].sum())
    # k' of a class is k + ITS largest count, not the class bound
    (c,) = [c for c in excl.plan_classes(torch.tensor([3, 9, 0]), 10, 1000) if c.count]
    assert c.k_search == 19 and c.rows.tolist() == [0, 1]
    # clamped at n_candidates
    classes = excl.plan_classes(torch.tensor([0, 35, 2]), 10, 40)
    assert [(c.count, c.k_search) for c in classes] == [(0, 10), (2, 12), (35, 40)]
    # all zero (or no query at all): one class, k' = k
    for counts in (torch.zeros(7, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)):
        (c,) = excl.plan_classes(counts, 25, 1000)
        assert c.k_search == 25 and c.count == 0 and c.rows.tolist() == list(range(counts.numel()))


def test_plan_classes_limit():
    excl.plan_classes(torch.tensor([3900]), 100, 10 ** 6)  # k + count = 4000: allowed
    with pytest.raises(ValueError, match="4000"):
        excl.plan_classes(torch.tensor([0, 3901]), 100, 10 ** 6)
    with pytest.raises(ValueError, match="4000"):
        excl.plan_classes(np.array([1]), 4000, 10 ** 6)
    with pytest.raises(ValueError):
        excl.plan_classes(torch.tensor([0]), 50, 40)  # k > n_candidates


# --------------------------------------------------------------------------- positions_of
def test_positions_of_integers_and_strings():
    ident = torch.tensor([40, 7, 19, 3, 1000, 8])
    pos = excl.positions_of(ident, torch.tensor([7, 1000, 5, 3, 40, -1, 2000]))
    assert pos.dtype == torch.int32 and pos.tolist() == [1, 4, -1, 3, 0, -1, -1]
    assert excl.positions_of(ident, [8, 9]).tolist() == [5, -1]
    assert excl.positions_of(ident, []).tolist() == []
    names = np.array(["0108775015", "a", "b b", "77"])
    pos = excl.positions_of(names, ["b b", "nope", "0108775015", 77, b"a", ""])
    assert pos.dtype == torch.int32 and pos.tolist() == [2, -1, 0, 3, 1, -1]
    m = excl.IdentifierMap(names)
    off, idx = excl.identifier_csr(m, [["a", "zz"], [], ["77", "b b", "q"]], 3)
    assert off.tolist() == [0, 1, 1, 3] and idx.tolist() == [1, 3, 2]  # unknown identifiers dropped
    off, idx = excl.identifier_csr(excl.IdentifierMap(ident), torch.tensor([[7, -5], [8, 40]]), 2)
    assert off.tolist() == [0, 1, 3] and idx.tolist() == [1, 5, 0]


# --------------------------------------------------------------------------- run_classes on the CPU oracle
def _oracle_run(c, k):
    from oracle import oracle

    def run(qc, k_search, off, idx, count):
        s, i, _ = oracle.bruteforce_topk(qc.numpy(), c, k_search)
        if count == 0:
            return torch.from_numpy(s), torch.from_numpy(i)
        s, i, _, _ = ref.exclude_lists(s, i, off.numpy(), idx.numpy(), k)
        return torch.from_numpy(s), torch.from_numpy(i)

    return run


def test_run_classes_equals_filtered_topk():
    from oracle import oracle

    rng = np.random.default_rng(3)
    c = rng.standard_normal((400, 8)).astype(np.float32)
    c[200:210] = c[5:15]
    q = rng.standard_normal((23, 8)).astype(np.float32)
    counts = [0, 3, 20, 70, 0, 300, 16, 17] * 3
    rows = [rng.choice(400, n, replace=False).tolist() for n in counts[:23]]
    rows[5] = list(range(395))  # k' clamps at 400 and only 5 candidates remain: padded
    k = 12
    s, i = excl.run_classes(torch.from_numpy(q), k, 400, rows, _oracle_run(c, k))
    rs, ri = ref.filtered_topk(oracle.fmaf_scores(q, c), rows, k)
    assert np.array_equal(i.numpy(), ri) and np.array_equal(s.numpy().view(np.int32), rs.view(np.int32))
    assert (ri[5, 5:] == PAD).all() and (ri[5, :5] != PAD).all()
    # no exclusions anywhere: the plain search's answer
    s0, i0 = excl.run_classes(torch.from_numpy(q), k, 400, [[]] * 23, _oracle_run(c, k))
    ps, pi, _ = oracle.bruteforce_topk(q, c, k)
    assert np.array_equal(i0.numpy(), pi) and np.array_equal(s0.numpy(), ps)


# --------------------------------------------------------------------------- sharded, over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cpu_index_ops(calls):
    from oracle import oracle
    from pkg.modelling.distributed import IndexOps

    def search(img, cand, q, k, off):
        s, i, _ = oracle.bruteforce_topk(q.numpy(), cand.numpy(), k)
        return torch.from_numpy(s), torch.from_numpy(i + off)

    def merge(s, i, k):
        ms, mi = oracle.topk_merge(s.numpy(), i.numpy(), k)
        return torch.from_numpy(np.ascontiguousarray(ms)), torch.from_numpy(np.ascontiguousarray(mi))

    def exclude(s, i, off, idx, k_out):
        calls.append((tuple(s.shape), k_out))
        os_, oi, kept, _ = ref.exclude_lists(s.numpy(), i.numpy(), off.numpy(), idx.numpy(), k_out)
        return torch.from_numpy(os_), torch.from_numpy(oi), torch.from_numpy(kept)

    return IndexOps(build=lambda c: None, search=search, merge=merge, exclude=exclude)


def _gloo_worker(rank, world, port, q, c, k, rows, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pkg.modelling.distributed import QueryShardedBruteForceIndex, ShardedBruteForceIndex, shard_range

    N = c.shape[0]
    tq = torch.from_numpy(q)
    # ragged: the first shard has 3 rows, fewer than every k' (its lists are padded)
    ragged = [3] + [(N - 3) // (world - 1) + (1 if r < (N - 3) % (world - 1) else 0) for r in range(world - 1)]
    for mode in ("even", "ragged"):
        if mode == "even":
            b, e = shard_range(N, world, rank)
        else:
            b, e = sum(ragged[:rank]), sum(ragged[:rank + 1])
        calls = []
        idx = ShardedBruteForceIndex(k, None, torch.from_numpy(c[b:e].copy()), ops=_cpu_index_ops(calls))
        s, i = idx.search(tq, exclusions=rows)
        blk, os_, oi = idx.search_owned(tq, exclusions=rows)
        p_s, p_i = idx.search(tq)  # exclusions=None: today's call
        out[(mode, rank)] = (s.numpy(), i.numpy(), blk, os_.numpy(), oi.numpy(), p_s.numpy(), p_i.numpy(), calls)
    calls = []
    qidx = QueryShardedBruteForceIndex(k, None, torch.from_numpy(c), ops=_cpu_index_ops(calls))
    s, i = qidx.search(tq, exclusions=rows)
    blk, os_, oi = qidx.search_owned(tq, exclusions=rows)
    out[("q", rank)] = (s.numpy(), i.numpy(), blk, os_.numpy(), oi.numpy())
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_exclusions_equal_filtered_topk(world):
    from oracle import oracle

    rng = np.random.default_rng(11)
    N, Q, k = 301, 22, 25
    c = np.maximum(rng.standard_normal((N, 16)), 0).astype(np.float32)
    c[100:140] = c[99]  # ties across shard boundaries, some of them excluded
    q = np.maximum(rng.standard_normal((Q, 16)), 0).astype(np.float32)
    q[3] = 0.0
    q[7] = rng.standard_normal(16).astype(np.float32)
    full = oracle.fmaf_scores(q, c)
    _, top, _ = oracle.bruteforce_topk(q, c, 2 * k)
    counts = [0, 5, 16, 30, 70, 0, 2, 40] * 3
    rows = []
    for qi in range(Q):  # drawn from the query's own top-2k: they reach across the shards and always bite
        n = counts[qi]
        own = rng.choice(top[qi], min(n, 2 * k), replace=False).tolist()
        if n:
            own[0] = int(top[qi, rng.integers(k)])  # at least one inside the unfiltered top-k (may repeat another)
        rows.append(own + rng.choice(N, n - len(own), replace=False).tolist())
    rows[3] = [0, 2] + list(range(95, 125))  # the all-ties query (every score 0) loses positions 0 and 2
    rs, ri = ref.filtered_topk(full, rows, k)
    assert all(not r or set(r) & set(top[qi, :k].tolist()) for qi, r in enumerate(rows))
    ps, pi, _ = oracle.bruteforce_topk(q, c, k)
    out = mp.Manager().dict()
    mp.spawn(_gloo_worker, args=(world, _free_port(), q, c, k, rows, out), nprocs=world, join=True)
    for r in range(world):
        for mode in ("even", "ragged"):
            s, i, (b, e), os_, oi, p_s, p_i, calls = out[(mode, r)]
            assert np.array_equal(i, ri) and np.array_equal(s.view(np.int32), rs.view(np.int32)), (mode, r)
            assert np.array_equal(oi, ri[b:e]) and np.array_equal(os_, rs[b:e]), (mode, r)
            assert np.array_equal(p_i, pi) and np.array_equal(p_s, ps)
            assert calls and all(k_out == k and shape[1] > k for shape, k_out in calls)
        s, i, (b, e), os_, oi = out[("q", r)]
        assert np.array_equal(i, ri) and np.array_equal(s, rs)
        assert np.array_equal(oi, ri[b:e]) and np.array_equal(os_, rs[b:e])


# --------------------------------------------------------------------------- IndexRecall
def test_index_recall_forwards_exclusions():
    from pkg.modelling.metrics.index_recall import IndexRecall

    seen = []

    def index(*args, **kwargs):
        seen.append((args, kwargs))
        return np.array([["a", "b"], ["c", "d"]], dtype=object)

    m = IndexRecall(index, [1, 2])
    queries = {"customer_id": ["x", "y"]}
    m(queries, np.array(["b", "c"], dtype=object))
    assert seen[-1] == ((queries,), {})  # one positional argument, as before
    r = m(queries, np.array(["b", "c"], dtype=object), exclusions=[["a"], []])
    assert seen[-1] == ((queries,), {"exclusions": [["a"], []]})
    assert r[1] == 0.5 and r[2] == 1.0 and m.seen == 4
