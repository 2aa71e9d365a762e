"""GPU: the exact top-k with per-query exclusions.

* tt_topk_exclude against the numpy restatement (tests/topk_exclude_ref.py):
  scores as int32 bit patterns, indices and n_kept exactly, over both launch
  forms (one wave per query up to k_in = 256, one workgroup per query above),
  a ragged last workgroup, and every kind of exclusion row.
* BruteForceIndex.search(exclusions=...) against the exact filtered top-k of
  the fp32 fmaf-chain scores, bit-exact; the identifier-level entry points;
  the Retriever on a saved index with string identifiers.
* the two sharded indices (two processes on cuda:0 over gloo) against the
  single-GPU search(exclusions=...).
"""
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import topk_exclude_ref as ref
from oracle import oracle
from pkg import _native
from pkg.modelling import hip_ops
from pkg.modelling.indices.brute_force import BruteForceIndex

PAD = ref.PAD_INDEX
SWITCH = 256  # largest k_in of the one-wave-per-query form (kExcludeSmallK)
K_INS = [1, 63, 64, 65, 200, SWITCH - 1, SWITCH, SWITCH + 1, 1000, 4096]
N_QUERIES = [1, 5, 9]
KINDS = 9


def _k_outs(k_in):
    return sorted({1, max(1, k_in // 2), k_in})


@functools.lru_cache(maxsize=None)
def _case(nq, k_in):
    """(scores [nq, k_in], idx [nq, k_in], exclusion rows) — row q is of kind
    (q + position of k_in in K_INS) % 9, so nine queries hold every kind and
    the single-query cases walk through them."""
    rng = np.random.default_rng(1000 * nq + k_in)
    P = 2
    while P < 2 * k_in:
        P *= 2
    scores = np.empty((nq, k_in), np.float32)
    idx = np.empty((nq, k_in), np.int32)
    rows = []
    for q in range(nq):
        kind = (q + K_INS.index(k_in)) % KINDS
        # descending scores with runs of equal values, a -0.0 / +0.0 pair and real -inf entries
        s = np.sort(rng.integers(-6, 7, k_in).astype(np.float32) * 0.5)[::-1].copy()
        s[np.flatnonzero(s == 0)[::2]] = -0.0
        n_inf = int(rng.integers(0, 3)) if k_in > 4 else 0
        n_pad = int(rng.integers(1, 4)) if (k_in > 8 and q % 2 == 1) else 0  # padded input tail
        real = k_in - n_pad
        if n_inf:
            s[real - n_inf:real] = -np.inf
        if kind == 8:  # list indices congruent modulo the table size
            i = (7 + np.arange(k_in, dtype=np.int64) * P)
        else:
            i = rng.choice(60000, k_in, replace=False).astype(np.int64)
        if n_pad:
            s[real:] = -np.inf
            i[real:] = PAD
        scores[q], idx[q] = s, i.astype(np.int32)
        inside = i[:real]
        outside = 70000 + rng.choice(60000, 3 * k_in + 8, replace=False)  # never in a list
        if kind == 0:
            e = []
        elif kind == 1:
            e = [inside[0]]
        elif kind == 2:
            e = [inside[-1]]
        elif kind == 3:
            e = rng.permutation(inside).tolist()  # the whole list: n_kept counts only input padding
        elif kind == 4:
            e = outside[:k_in + 3].tolist()
        elif kind == 5:
            hit = inside[rng.integers(0, real, 3)]
            e = np.concatenate([hit, hit, hit[:1], outside[:2], outside[:2]]).tolist()
        elif kind == 6:
            e = [-1, PAD, -PAD, inside[real // 2], -int(inside[0]) - 1, PAD, -2 ** 31]
        elif kind == 7:  # far more exclusions than entries: 5000 against k_in = 65
            n = 5000 if k_in == 65 else 3 * k_in + 5
            e = np.concatenate([70000 + rng.choice(10 ** 6, n - real // 2 - 1, replace=False),
                                rng.choice(inside, real // 2 + 1, replace=False)])
            e = rng.permutation(e).tolist()
        else:  # same residue modulo the table size: hits, and misses that probe through the hits' slots
            e = np.concatenate([i[:real:2], 7 + (k_in + np.arange(k_in // 2 + 1, dtype=np.int64)) * P]).tolist()
        rows.append([int(v) for v in e])
    return scores, idx, rows


@functools.lru_cache(maxsize=None)
def _case_ref(nq, k_in, k_out):
    scores, idx, rows = _case(nq, k_in)
    off, flat = ref.csr_of(rows)
    return ref.exclude_lists(scores, idx, off, flat, k_out)


def test_kernel_cases_reach_padding_and_full_hit_rows():
    """On the helper alone: the parametrised cases hold a row with fewer than
    k_out survivors (padding written), a row whose every exclusion hits, rows
    with input padding, tied scores and real -inf scores."""
    short = full_hit = padded_in = ties = infs = 0
    for nq in N_QUERIES:
        for k_in in K_INS:
            scores, idx, rows = _case(nq, k_in)
            padded_in += int((idx == PAD).any())
            ties += int((scores[:, 1:] == scores[:, :-1]).any())
            infs += int(np.isinf(scores[idx != PAD]).any())
            for k_out in _k_outs(k_in):
                _, _, kept, surv = _case_ref(nq, k_in, k_out)
                short += int((surv < k_out).sum())
                assert np.array_equal(kept, np.minimum(surv, k_out))
            for q, r in enumerate(rows):
                full_hit += int(bool(r) and set(r) <= set(idx[q].tolist()) - {PAD})
    assert short >= 1 and full_hit >= 1 and padded_in >= 1 and ties >= 1 and infs >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("k_in", K_INS)
@pytest.mark.parametrize("nq", N_QUERIES)
def test_topk_exclude_matches_helper(cuda, nq, k_in):
    scores, idx, rows = _case(nq, k_in)
    off, flat = ref.csr_of(rows)
    ts, ti = torch.as_tensor(scores, device=cuda), torch.as_tensor(idx, device=cuda)
    toff, tflat = torch.as_tensor(off, device=cuda), torch.as_tensor(flat, device=cuda)
    for k_out in _k_outs(k_in):
        rs, ri, rkept, _ = _case_ref(nq, k_in, k_out)
        s, i, kept = hip_ops.topk_exclude(ts, ti, toff, tflat, k_out)
        assert tuple(s.shape) == (nq, k_out) and s.dtype == torch.float32 and i.dtype == torch.int32
        assert np.array_equal(kept.cpu().numpy(), rkept), (k_out, kept.cpu().numpy(), rkept)
        assert np.array_equal(i.cpu().numpy(), ri), k_out
        assert np.array_equal(s.cpu().numpy().view(np.int32), rs.view(np.int32)), k_out
    # the inputs were only read
    assert np.array_equal(ts.cpu().numpy().view(np.int32), scores.view(np.int32))
    assert np.array_equal(ti.cpu().numpy(), idx)


@pytest.mark.gpu
def test_topk_exclude_without_n_kept_and_with_no_exclusions(cuda):
    """The C ABI with n_kept = NULL, and excl_idx = NULL when every list is
    empty: the copy-only path returns the first k_out entries."""
    scores, idx, _ = _case(9, 200)
    ts, ti = torch.as_tensor(scores, device=cuda), torch.as_tensor(idx, device=cuda)
    off = torch.zeros(10, dtype=torch.int64, device=cuda)
    os_ = torch.empty(9, 50, dtype=torch.float32, device=cuda)
    oi = torch.empty(9, 50, dtype=torch.int32, device=cuda)
    _native.check(_native.lib().tt_topk_exclude(ts.data_ptr(), ti.data_ptr(), 9, 200, 50, off.data_ptr(), None,
                                                os_.data_ptr(), oi.data_ptr(), None,
                                                torch.cuda.current_stream().cuda_stream))
    assert np.array_equal(oi.cpu().numpy(), idx[:, :50])
    assert np.array_equal(os_.cpu().numpy().view(np.int32), scores[:, :50].view(np.int32))
    s, i, kept = hip_ops.topk_exclude(ts, ti, off, torch.zeros(0, dtype=torch.int32, device=cuda), 200)
    assert kept.tolist() == [200] * 9 and np.array_equal(i.cpu().numpy(), idx)
    with pytest.raises(ValueError):
        hip_ops.topk_exclude(ts, ti, off, torch.zeros(0, dtype=torch.int32, device=cuda), 201)
    with pytest.raises(TypeError):
        hip_ops.topk_exclude(ts, ti, off.to(torch.int32), torch.zeros(0, dtype=torch.int32, device=cuda), 5)


# --------------------------------------------------------------------------- end to end
N, Q = 3001, 130
COUNT_CYCLE = [0, 3, 16, 40, 100, 0, 64, 150]  # classes 0, <= 16, <= 64, <= 256


@functools.lru_cache(maxsize=None)
def _problem(dim, signed):
    """Candidates, queries, the full fp32 fmaf-chain score matrix and each
    query's unfiltered top-300 — computed once and shared, never modified."""
    rng = np.random.default_rng(dim + 7 * signed)
    c = rng.standard_normal((N, dim)).astype(np.float32)
    q = rng.standard_normal((Q, dim)).astype(np.float32)
    if not signed:
        c, q = np.maximum(c, 0), np.maximum(q, 0)
    c[2000:2030] = c[20:50]  # ties that straddle excluded and kept rows
    q[0] = 0.0               # every score ties at 0
    full = oracle.fmaf_scores(q, c)
    _, top, _ = oracle.bruteforce_topk(q, c, 300)
    for a in (c, q, full, top):
        a.setflags(write=False)
    return c, q, full, top


def _exclusion_rows(top, k, seed):
    """Per query, COUNT_CYCLE[q % 8] exclusions drawn from its own unfiltered
    top-2k (and beyond it once 2k runs out), at least one inside the top-k."""
    rng = np.random.default_rng(seed)
    rows = []
    for qi in range(Q):
        n = COUNT_CYCLE[qi % len(COUNT_CYCLE)]
        if n == 0:
            rows.append([])
            continue
        pool = top[qi, :max(2 * k, n)]
        r = rng.choice(pool, n, replace=False).tolist()
        r[0] = int(top[qi, rng.integers(min(k, 20))])
        if qi % 3 == 0:  # each member of a tied pair (rows 20..49 = rows 2000..2029), where one is in reach
            twins = [int(v) for v in pool if 20 <= v < 50 or 2000 <= v < 2030]
            r[1:1 + len(twins[:2])] = twins[:2]
        rows.append([int(v) for v in r])
    rows[0] = [0, 2]  # the all-zero query: every score ties, positions 0 and 2 go
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("dim", [32, 100, 128])
@pytest.mark.parametrize("k", [10, 100])
def test_search_with_exclusions_is_the_exact_filtered_topk(cuda, k, dim, signed):
    c, q, full, top = _problem(dim, signed)
    rows = _exclusion_rows(top, k, 5)
    # asserted on the oracle before the GPU is looked at: every non-empty list bites
    for qi, r in enumerate(rows):
        assert not r or set(r) & set(top[qi, :k].tolist()), qi
    assert len({min(len(r), 1) + (len(r) > 16) + (len(r) > 64) for r in rows}) == 4  # four classes
    rs, ri = ref.filtered_topk(full, rows, k)
    index = BruteForceIndex(k, None, [(torch.arange(N, dtype=torch.int32), torch.tensor(c))], device=cuda)
    tq = torch.tensor(q, device=cuda)
    s, i = index.search(tq, exclusions=rows)
    assert np.array_equal(i.cpu().numpy(), ri)
    assert np.array_equal(s.cpu().numpy().view(np.int32), rs.view(np.int32))
    # the count-0 class is the plain search, bit for bit
    ps, pi = index.search(tq)
    none = [qi for qi, r in enumerate(rows) if not r]
    assert torch.equal(i[none], pi[none]) and torch.equal(s[none].view(torch.int32), ps[none].view(torch.int32))
    # the same exclusions as a padded device tensor and as an (off, idx) pair
    width = max(len(r) for r in rows)
    padded = torch.full((Q, width), -1, dtype=torch.int32)
    for qi, r in enumerate(rows):
        padded[qi, :len(r)] = torch.tensor(r, dtype=torch.int32)
    off, flat = ref.csr_of(rows)
    for form in (padded.to(cuda), (torch.as_tensor(off), torch.as_tensor(flat))):
        s2, i2 = index.search(tq, exclusions=form)
        assert torch.equal(i2, i) and torch.equal(s2.view(torch.int32), s.view(torch.int32))


@pytest.mark.gpu
def test_uniform_counts_and_identifier_level(cuda):
    """One class for the whole batch (no gather / scatter), and
    query_with_exclusions / call on integer identifiers."""
    c, q, full, top = _problem(32, True)
    k = 10
    ident = torch.arange(N, dtype=torch.int64) * 3 + 11
    index = BruteForceIndex(k, lambda x: x["emb"], [(ident, torch.tensor(c))], device=cuda)
    rows = [top[qi, [0, 3, 7, 15]].tolist() for qi in range(Q)]
    rs, ri = ref.filtered_topk(full, rows, k)
    tq = torch.tensor(q, device=cuda)
    s, i = index.search(tq, exclusions=rows)
    assert np.array_equal(i.cpu().numpy(), ri) and np.array_equal(s.cpu().numpy().view(np.int32), rs.view(np.int32))
    by_id = [[3 * v + 11 for v in r] + [5, -4] for r in rows]  # 5 and -4 are no identifiers: ignored
    got, gs = index.query_with_exclusions({"emb": tq}, by_id, scores=True)
    assert np.array_equal(got.cpu().numpy(), 3 * ri.astype(np.int64) + 11) and torch.equal(gs, s)
    assert torch.equal(index({"emb": tq}, exclusions=by_id), got)
    assert torch.equal(index.call({"emb": tq}, exclusions=by_id), got)
    assert torch.equal(index({"emb": tq}), index.lookup_identifiers(index.search(tq)[1]))


@pytest.mark.gpu
def test_padding_and_limits(cuda):
    rng = np.random.default_rng(2)
    c = rng.standard_normal((40, 16)).astype(np.float32)
    q = rng.standard_normal((6, 16)).astype(np.float32)
    index = BruteForceIndex(10, lambda x: x["emb"], [(torch.arange(40), torch.as_tensor(c))], device=cuda)
    rows = [[], [1, 2], list(range(35)), [39], [], list(range(5, 40))]
    rs, ri = ref.filtered_topk(oracle.fmaf_scores(q, c), rows, 10)
    tq = torch.as_tensor(q, device=cuda)
    s, i = index.search(tq, exclusions=rows)
    assert np.array_equal(i.cpu().numpy(), ri) and np.array_equal(s.cpu().numpy().view(np.int32), rs.view(np.int32))
    assert (ri[2, 5:] == PAD).all() and np.isinf(rs[2, 5:]).all() and (ri[2, :5] >= 35).all()  # search pads the row
    with pytest.raises(ValueError, match="40"):
        index.query_with_exclusions({"emb": tq}, rows)
    # k + count > 4000 is refused before anything is launched
    big = BruteForceIndex(100, None, [(torch.arange(5000), torch.zeros(5000, 16))], device=cuda)
    launched = []
    orig = hip_ops.bruteforce_search
    hip_ops.bruteforce_search = lambda *a, **kw: launched.append(1) or orig(*a, **kw)
    try:
        with pytest.raises(ValueError, match="4000"):
            big.search(torch.zeros(3, 16, device=cuda), exclusions=[[], list(range(3901)), [1]])
    finally:
        hip_ops.bruteforce_search = orig
    assert not launched


# --------------------------------------------------------------------------- serving
@pytest.mark.gpu
def test_retriever_excludes_raw_string_identifiers(cuda, tmp_path):
    from pkg import dtypes
    from pkg.modelling.export import Retriever
    from pkg.modelling.models.tower import Tower
    from pkg.schema.features import Feature, FeatureFamily

    V = [str(v) for v in range(200)]
    tower = Tower([Feature("cust", dtypes.string, FeatureFamily.QUERY, embedding_size=16, vocab=V)], 32, [48], cuda)
    rng = np.random.default_rng(4)
    cand = rng.standard_normal((300, 32)).astype(np.float32)
    ids = np.array([f"article-{a}" for a in range(300)])
    index = BruteForceIndex(10, tower, [(ids, torch.as_tensor(cand))], device=cuda)
    index.save(str(tmp_path / "i"))
    served = Retriever.load(str(tmp_path / "i"), device=cuda)
    raw = {"cust": [str(x) for x in rng.integers(0, 220, 48)]}
    plain, plain_s = served(raw, scores=True)
    assert np.array_equal(served(raw, exclude=None), plain)  # today's result
    emb = tower(tower.input_layer.encode(raw)).cpu().numpy()
    full = oracle.fmaf_scores(emb, cand)
    _, top, _ = oracle.bruteforce_topk(emb, cand, 10)
    assert np.array_equal(plain, ids[top])
    rows = [[] if b % 4 == 0 else top[b, :1 + b % 7].tolist() for b in range(48)]
    exclude = [[f"article-{v}" for v in r] + (["no-such-article"] if b % 3 == 0 else []) for b, r in enumerate(rows)]
    rs, ri = ref.filtered_topk(full, rows, 10)
    got, gs = served(raw, scores=True, exclude=exclude)
    assert np.array_equal(got, ids[ri]) and np.array_equal(gs.cpu().numpy().view(np.int32), rs.view(np.int32))
    got5 = served(raw, k=5, exclude=exclude)
    assert np.array_equal(got5, ids[ri[:, :5]])
    # integers are compared as their str() text, like the query features
    assert index.exclusion_positions([[7, "8"]], 1)[1].tolist() == []  # "7" and "8" are no identifiers here
    assert index.exclusion_positions([["article-7", "zzz"]], 1)[1].tolist() == [7]


# --------------------------------------------------------------------------- sharded
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sharded_worker(rank, world, port, c, q, k, rows, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "hm-retrieval-two-tower_amd")]
    from pkg.modelling.distributed import QueryShardedBruteForceIndex, ShardedBruteForceIndex, shard_range

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    tq = torch.as_tensor(q, device=dev)
    b, e = shard_range(c.shape[0], world, rank)
    idx = ShardedBruteForceIndex(k, None, torch.as_tensor(c[b:e], device=dev))  # this rank's rows only
    s, i = idx.search(tq, exclusions=rows)
    blk, os_, oi = idx.search_owned(tq, exclusions=rows)
    qidx = QueryShardedBruteForceIndex(k, None, torch.as_tensor(c, device=dev))
    qs, qi = qidx.search(tq, exclusions=rows)
    qblk, qos, qoi = qidx.search_owned(tq, exclusions=rows)
    torch.cuda.synchronize()
    out[rank] = tuple(x.cpu().numpy() if isinstance(x, torch.Tensor) else x
                      for x in (s, i, blk, os_, oi, qs, qi, qblk, qos, qoi))
    dist.destroy_process_group()


@pytest.mark.gpu
def test_sharded_indices_equal_single_gpu_search_with_exclusions(cuda):
    rng = np.random.default_rng(9)
    n, nq, k, world = 5003, 200, 50, 2
    c = np.maximum(rng.standard_normal((n, 32)), 0).astype(np.float32)
    c[2490:2520] = c[100:130]  # ties across the shard boundary (2502)
    q = np.maximum(rng.standard_normal((nq, 32)), 0).astype(np.float32)
    _, top, _ = oracle.bruteforce_topk(q, c, 2 * k)
    rows = []
    for qi in range(nq):  # up to 70 per query, from its own top-2k: both shards, always inside the top-k
        cnt = [0, 70, 9, 33, 0, 64, 17, 1][qi % 8]
        r = rng.choice(top[qi], cnt, replace=False).tolist()
        if cnt:
            r[0] = int(top[qi, rng.integers(k)])
        rows.append([int(v) for v in r])
    assert any(any(v < 2502 for v in r) and any(v >= 2502 for v in r) for r in rows)
    tc = torch.as_tensor(c, device=cuda)
    index = BruteForceIndex(k, None, [(torch.arange(n), tc)], device=cuda)
    ref_s, ref_i = index.search(torch.as_tensor(q, device=cuda), exclusions=rows)
    ref_s, ref_i = ref_s.cpu().numpy(), ref_i.cpu().numpy()
    sel = np.arange(0, nq, 9)
    os_, oi_ = ref.filtered_topk(oracle.fmaf_scores(q[sel], c), [rows[j] for j in sel], k)
    assert np.array_equal(ref_i[sel], oi_) and np.array_equal(ref_s[sel], os_)
    del tc, index
    out = mp.Manager().dict()
    mp.spawn(_sharded_worker, args=(world, _free_port(), c, q, k, rows, out), nprocs=world, join=True)
    covered = []
    for r in range(world):
        s, i, (b, e), bs, bi, qs, qi_, (qb, qe), qos, qoi = out[r]
        assert np.array_equal(i, ref_i) and np.array_equal(s.view(np.int32), ref_s.view(np.int32))
        assert np.array_equal(bi, ref_i[b:e]) and np.array_equal(bs, ref_s[b:e])
        assert np.array_equal(qi_, ref_i) and np.array_equal(qs.view(np.int32), ref_s.view(np.int32))
        assert (qb, qe) == (b, e) and np.array_equal(qoi, ref_i[b:e]) and np.array_equal(qos, ref_s[b:e])
        covered += list(range(b, e))
    assert covered == list(range(nq))
